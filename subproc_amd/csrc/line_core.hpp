// line_core.hpp — the PRINCIPAL VARIATION: the line of best play behind a
// value, a thin layer around solve_core.hpp's advance() and search_core.hpp's
// advance() / order_core.hpp's advance_ordered(), written once for the device
// (line.hip) and the host (tools/diag/line_host.cpp).  include/othello_line.h
// states the rule; DESIGN.md §24 has the argument.
//
// The layer is one more transition of the lane's machine, where budget_core.hpp
// puts deepen(): when the lane's search ends (Lane::depth < 0) with value v and
// move m, follow() records m, plays it with the machine's own rules R and
// restarts the lane on the child AS A ROOT OF ITS OWN with the window narrowed
// to (-v - 1, -v + 1), or retires the lane.  Every node of the line is then a
// root, so "the lowest maximiser" holds at every ply by the rule the machines
// already have, with or without move ordering.  A forced pass is a root whose
// search answers 64: it is recorded and played like a move.
//
// Why the window: the child's value is -v, strictly inside it, so the search is
// exact there; and for a fixed move order alpha-beta on a window inside the one
// the parent's search gave the child visits a subset of its nodes, so no
// follow-up search meets a node limit the root search did not.
//
// A lane's state beyond its Lane: Walk below (the position the walk stands at,
// the root's answer, the nodes' sum, the line's length).  The line's bytes go
// to `out` as they are settled: out.move(k, code) records entry k,
// out.clear(len) takes a line back (an answer at a limit is all or nothing).
#pragma once
#include <stdint.h>

#include "order_core.hpp"
#include "search_core.hpp"
#include "solve_core.hpp"

namespace othl {

using othm::u32;
using othm::u64;

constexpr int kLineStride = 32;  // OTHL_LINE_STRIDE
constexpr u32 kBadDepth = 6;     // OTHL_BADDEPTH
constexpr u32 kNoMove = 255, kPassMove = 64;
static_assert(oths::kNoMove == kNoMove && othm::kNoMove == kNoMove && oths::kPassMove == kPassMove &&
                  othm::kPassMove == kPassMove && oths::kLimit == othm::kLimit,
              "the solver's and the search's codes are one set here");

struct Walk {
    u64 P, O;     // the position the walk stands at: the mover's discs, the other side's
    u64 nodes;    // of the walk's searches so far
    int value;    // the root's answer, from the root mover's side
    u32 move;
    u32 status;
    u32 len;      // entries of the line
    int rem;      // the search: plies left at (P, O); the solver: unused
    bool first;   // the running search is the root's
    bool root_side;  // the root mover is to move at (P, O)
};

OTHM_FN void open(Walk& W, u64 P, u64 O, int plies, u32 status) {
    W.P = P;
    W.O = O;
    W.nodes = 0;
    W.value = 0;
    W.move = kNoMove;
    W.status = status;
    W.len = 0;
    W.rem = plies;
    W.first = true;
    W.root_side = true;
}

OTHM_FN u32 nodes32(const Walk& W) { return W.nodes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)W.nodes; }

// the part of follow() both machines share: the ended search's answer (value v
// for the walk's mover, move m, status) goes into the walk and m is played.
// True: the walk goes on from the new (P, O), whose mover's value is -v.
template <class R, class Out>
OTHM_FN bool advance_walk(Walk& W, int v, u32 m, u32 status, u32 nodes, Out& out) {
    W.nodes += nodes;
    if (status == othm::kLimit) {  // all or nothing
        out.clear(W.len);
        W.len = 0;
        W.value = 0;
        W.move = kNoMove;
        W.status = status;
        return false;
    }
    if (W.first) {
        W.value = v;
        W.move = m;
        W.first = false;
    }
    // 255: the game is over here (the value is strictly inside a follow-up
    // window, so a position with a move always names one); a full row: cannot be
    if (m == kNoMove || W.len >= (u32)kLineStride) return false;
    if (m == kPassMove) {
        const u64 p = W.P;
        W.P = W.O;
        W.O = p;
    } else {
        const u64 f = R::flips(m, W.P, W.O);
        const u64 p = W.O & ~f;
        W.O = W.P | f | (1ull << m);
        W.P = p;
        W.rem--;
    }
    out.move(W.len, m);
    W.len++;
    W.root_side = !W.root_side;
    return true;
}

// THE SOLVER.  begin_solve() then oths::advance() until L.depth < 0, then
// follow_solve(): true = the lane is searching again, false = the walk is over
// and W holds the answer.  The boards are disjoint and within max_empties
// (classified by the caller).
OTHM_FN void begin_solve(Walk& W, oths::Lane& L, u64 P, u64 O) {
    open(W, P, O, 0, oths::kSolved);
    oths::start(L, P, O);
}

template <class R, class Out>
OTHM_FN bool follow_solve(Walk& W, oths::Lane& L, Out& out) {
    const int v = L.value;
    if (!advance_walk<R>(W, v, L.best_mv, L.status, L.nodes, out)) return false;
    if (~(W.P | W.O) == 0) return false;  // the board is full: neither side can move
    oths::start(L, W.P, W.O, -v - 1, -v + 1);
    return true;
}

// THE SEARCH.  begin_search() with 1 <= plies <= othm::kMaxDepth, then
// othm::advance() / advance_ordered<R, true>() until L.depth < 0, then
// follow_search() (the caller resets its ordering state when it returns true).
OTHM_FN void begin_search(Walk& W, othm::Lane& L, u64 P, u64 O, int plies) {
    open(W, P, O, plies, othm::kSearched);
    othm::start(L, P, O, plies);
}

template <class R, class Out>
OTHM_FN bool follow_search(Walk& W, othm::Lane& L, Out& out) {
    const int v = L.value;
    if (!advance_walk<R>(W, v, L.best_mv, L.status, L.nodes, out)) return false;
    if (W.rem <= 0) return false;  // the leaf whose score the value is
    if (W.root_side)
        othm::start(L, W.P, W.O, W.rem);
    else
        othm::start_child(L, W.P, W.O, R::moves(W.P, W.O), W.rem);
    L.alpha = -v - 1;
    L.beta = -v + 1;
    return true;
}

// what a per-position depth is before any search: kSearched = search it
OTHM_FN u32 classify_depth(u32 depth) {
    return depth == 0 ? othm::kLimit : depth > (u32)othm::kMaxDepth ? kBadDepth : othm::kSearched;
}

}  // namespace othl
