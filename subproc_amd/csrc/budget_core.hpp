// budget_core.hpp — search by NODE BUDGET: iterative deepening around
// search_core.hpp's advance() and order_core.hpp's advance_ordered(), written
// once for the device (budget.hip) and the host (tools/diag/budget_host.cpp).
// include/othello_budget.h states the rule; DESIGN.md §22 has the argument.
//
// The deepening layer is one more transition of the lane's machine, where
// play_core.hpp's advance() puts step(): when the lane's search ends
// (Lane::depth < 0) the layer either restarts the lane one ply deeper with
// othm::start() (which zeroes Lane::nodes) and the reduced limit, or retires the
// lane with the answer of the deepest iteration that completed.  The limit is
// passed to advance() by value, so a per-lane limit is a register (Deepen::rem).
// Iterations share nothing: iteration d IS the fixed-depth search at depth d.
//
// A lane's state beyond its Lane: the root's boards (the caller's: the search
// kernel keeps them, a game already has them), and Deepen below.
//
// The game driver, advance_play(), is play_core.hpp's advance() with the layer
// between the search and step(): step() starts every search as it always did;
// where the budget applies, the layer turns the search just started into
// iteration 1, and when the iterations are over it writes the recorded answer
// into the Lane, where step() reads the finished search's.
#pragma once
#include <stdint.h>

#include "order_core.hpp"
#include "play_core.hpp"
#include "search_core.hpp"

namespace othb {

using othm::u32;
using othm::u64;

struct Deepen {
    u32 rem;    // nodes left for the running iteration and those after it
    int d;      // the running iteration's depth; 0: the lane's search is not a budget search
    int last;   // K: the last iteration's depth
    // the answer of the deepest completed iteration
    int value;
    u32 move;
    u32 depth;  // 0: none completed
    u32 nodes;  // the completed iterations' nodes
};

// K = min(cap, max(1, empties)): a pass costs no depth, so depth `empties`
// already searches the whole tree
template <class R>
OTHM_FN int last_depth(u64 P, u64 O, int cap) {
    int e = 64 - R::count(P | O);
    e = e < 1 ? 1 : e;
    return cap < e ? cap : e;
}

// the deepening state of a root with `budget` nodes; the caller starts (or has
// started) the lane's search at depth 1
template <class R>
OTHM_FN void open(Deepen& D, u64 P, u64 O, u32 budget, int cap) {
    D.rem = budget;
    D.d = 1;
    D.last = last_depth<R>(P, O, cap);
    D.value = 0;
    D.move = othm::kNoMove;
    D.depth = 0;
    D.nodes = 0;
}

// the running iteration has ended (L.depth < 0).  True: the next one has
// started (the caller resets its ordering state); false: the root is done and
// D holds its answer.
OTHM_FN bool deepen(Deepen& D, othm::Lane& L, u64 P, u64 O) {
    if (L.status == othm::kLimit) return false;  // needed more than rem: the answer stays the last one's
    D.value = L.value;
    D.move = L.best_mv;
    D.depth = (u32)D.d;
    D.nodes += L.nodes;
    D.rem -= L.nodes;  // (a completed search counted at most its limit)
    if (D.d >= D.last || D.rem == 0) return false;
    D.d++;
    othm::start(L, P, O, D.d);
    return true;
}

OTHM_FN u32 status_of(const Deepen& D) { return D.depth ? othm::kSearched : othm::kLimit; }

// ONE POSITION.  begin_search() then advance_search() until it returns true;
// the answer is D's and status_of(D).  The boards are disjoint (checked).
template <class R>
OTHM_FN void begin_search(Deepen& D, othm::Lane& L, u64 P, u64 O, u32 budget, int cap) {
    open<R>(D, P, O, budget, cap);
    if (budget)
        othm::start(L, P, O, 1);
    else
        L.depth = -1;  // a budget of 0: nothing is searched, the status is kLimit
}

// one step of the lane's budget search; requires L.depth >= 0.  True: done.
template <class R, bool kOrdered, class S>
OTHM_FN bool advance_search(Deepen& D, othm::Lane& L, othm::Order& Q, S& stk, const int* table, u64 P, u64 O) {
    if constexpr (kOrdered)
        othm::advance_ordered<R, true>(L, Q, stk, table, D.rem);
    else
        othm::advance<R>(L, stk, table, D.rem);
    if (L.depth >= 0) return false;
    if (!deepen(D, L, P, O)) return true;
    if constexpr (kOrdered) othm::order_reset(Q);
    return false;
}

// THE GAMES.  The players' budgets; index 0 is player A, 1 is player B.
struct Budgets {
    u32 budget[2];  // >= 1
};

// One step of a live game's lane: play_core.hpp's advance() with the deepening
// layer.  m.depth[] are the caps; m.limit bounds the searches without a budget
// (those at empties <= m.exact_empties).  D.d == 0 at a game's begin.
template <class R, bool kOrdered, bool kPark = false, class S, class Out>
OTHM_FN void advance_play(othp::Game& G, othm::Lane& L, othm::Order& Q, Deepen& D, S& stk, const int* tables,
                          const othp::Match& m, const Budgets& b, Out& out) {
    if (L.depth >= 0) {
        const u32 limit = D.d ? D.rem : m.limit;
        if constexpr (kOrdered)
            othm::advance_ordered<R, true>(L, Q, stk, tables + othm::kEvalTable * (int)othp::mover_player(G), limit);
        else
            othm::advance<R>(L, stk, tables + othm::kEvalTable * (int)othp::mover_player(G), limit);
        if (L.depth < 0 && D.d) {
            if (deepen(D, L, G.P, G.O)) {
                if constexpr (kOrdered) othm::order_reset(Q);
            } else {  // the answer, where step() reads a finished search's
                L.value = D.value;
                L.best_mv = D.move;
                L.status = status_of(D);
                L.nodes = D.nodes;
                D.d = 0;
            }
        }
    }
    if (L.depth < 0) {
        othp::step<R, kPark>(G, L, m, out);
        if constexpr (kOrdered) othm::order_reset(Q);
        if (L.depth >= 0 && 64 - R::count(G.P | G.O) > m.exact_empties) {
            // the search step() has just started becomes iteration 1 of the mover's budget
            const u32 player = othp::mover_player(G);
            open<R>(D, G.P, G.O, player ? b.budget[1] : b.budget[0], player ? m.depth[1] : m.depth[0]);
            L.rem = 1;
        }
    }
}

}  // namespace othb
