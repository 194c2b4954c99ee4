// play_solve_core.hpp — search self-play whose last plies are the exact
// solver's (include/othello_play_solve.h): what joins
// play_core.hpp's games to solve_core.hpp's machine, written once for the
// device (play_solve.hip) and the host (tools/diag/play_solve_host.cpp).
//
// A game runs in two phases.  The first is play_core.hpp's (budget_core.hpp's)
// loop with step<R, true>(): a game whose turn begins with at most E empty
// squares leaves it as othp::kParked, before any draw of that turn, and its
// state goes into a record (pack() below).  The second phase takes the records
// up (unpack()) and plays each game to its end with advance() below: the turn
// logic of othp::step() around oths::advance() in place of the search's.
//
// step() here restates the turn of othp::step() (game over / pass / coin /
// single move) rather than sharing its text: taking that text apart into pieces
// changed the instructions of play.hip's and budget.hip's kernels, which this
// change leaves as they were.  tests/test_play_solve_host.py holds the two
// statements together (the games at E <= 8 are the search's own).
//
// The window: when the move just played was the solver's own choice with value
// v, the position it leads to is worth -v to its mover, so a policy turn there
// solves on (-v - 1, -v + 1): exact there, and the lowest maximiser by the rule
// the machine already has (line_core.hpp).  After a coin move, a
// single move, a pass, or where the game comes in, the window is the full one.
#pragma once
#include <stdint.h>

#include "play_core.hpp"
#include "solve_core.hpp"

namespace othx {

using othm::u32;
using othm::u64;

static_assert(oths::kLimit == othm::kLimit && oths::kNoMove == othm::kNoMove && oths::kPassMove == othp::kPassMove,
              "the solver's and the search's codes are one set here");

constexpr int kRecordWords = 6;     // 64-bit words of a parked game: OTHX_PARKED_BYTES / 8
constexpr int kCounterWords = 2;    // the list's counter and its padding: OTHX_COUNTER_BYTES / 8

// a parked game's record: the boards, the RNG, the game's index in the launch,
// its nodes so far, and ply / budgets / colours in one word
OTHM_FN void pack(const othp::Game& G, u64 g, u64* w) {
    w[0] = G.P;
    w[1] = G.O;
    w[2] = (u64)G.rng.state | ((u64)G.rng.inc << 32);
    w[3] = g;
    w[4] = G.nodes;
    w[5] = (u64)(G.ply | (G.rem << 8) | (G.rem_other << 16) | ((u32)G.mover_black << 24) | ((u32)G.a_black << 25));
}

// the record's game, live and between two turns; the answer is its index
OTHM_FN u64 unpack(othp::Game& G, const u64* w) {
    const u32 f = (u32)w[5];
    G.P = w[0];
    G.O = w[1];
    G.rng.state = (u32)w[2];
    G.rng.inc = (u32)(w[2] >> 32);
    G.nodes = w[4];
    G.ply = f & 0xFFu;
    G.rem = (f >> 8) & 0xFFu;
    G.rem_other = (f >> 16) & 0xFFu;
    G.mover_black = (f >> 24) & 1u;
    G.a_black = (f >> 25) & 1u;
    G.live = true;
    G.next = othp::kMoveNone;
    G.status = othm::kSearched;
    return w[3];
}

// One step of a live game whose lane is not solving (L.depth < 0): othp::step()
// with the solver for rule 4.  The game has ended when G.live is false on
// return; a solve has started when L.depth >= 0.
template <class R, class Out>
OTHM_FN void step(othp::Game& G, oths::Lane& L, Out& out) {
    u32 mv = G.next;
    bool known = false;  // the move is the solver's own: the next position's value is -v
    int v = 0;
    if (mv == othp::kMoveSearch) {
        G.nodes += L.nodes;
        // (a solved root with two moves names one: the second test keeps a defect from playing on for ever)
        if (L.status == oths::kLimit || L.best_mv >= 64u) {
            G.status = othm::kLimit;
            G.live = false;
            return;
        }
        mv = L.best_mv;
        v = L.value;
        known = true;
    }
    G.next = othp::kMoveNone;
    if (G.ply >= othp::kMaxPlies) {
        G.status = othm::kLimit;
        G.live = false;
        return;
    }
    if (mv < 64u) {
        const u64 f = R::flips(mv, G.P, G.O);
        const u64 np = G.O & ~f;
        G.O = G.P | f | (1ull << mv);
        G.P = np;
        out.move(G.ply, mv);
        othp::hand_over(G);
    }
    const u64 own = R::moves(G.P, G.O);
    if (own == 0) {
        if (R::moves(G.O, G.P) == 0) {  // neither side can move: the game is over
            G.live = false;
            return;
        }
        if (G.rem) (void)G.rng.pick(G.rem);  // the passer's turn draws its coin too
        const u64 t = G.P;
        G.P = G.O;
        G.O = t;
        out.move(G.ply, othp::kPassMove);
        othp::hand_over(G);
        return;
    }
    const u32 cnt = (u32)R::count(own);
    if (G.rem && G.rng.pick(G.rem) == 0u) {  // the coin: a random legal move
        G.next = othp::kth_set_bit<R>(own, G.rng.pick(cnt));
        G.rem--;
        return;
    }
    if (cnt == 1u) {
        G.next = R::lowest(own);
        return;
    }
    // (empties only fall, so the position is within the zone it was parked in: at most oths::kMaxEmpties)
    oths::start(L, G.P, G.O, known ? -v - 1 : -oths::kInf, known ? -v + 1 : oths::kInf);
    // the root's move mask is known: enter the solve past its kRootNew step
    L.M = own;
    L.flags = 0;
    G.next = othp::kMoveSearch;
}

// One step of a live game's lane in the second phase: of its solve, and of the
// game when that leaves the lane without one.  `limit`: nodes per solve.
template <class R, class S, class Out>
OTHM_FN void advance(othp::Game& G, oths::Lane& L, S& stk, u32 limit, Out& out) {
    if (L.depth >= 0) oths::advance<R>(L, stk, limit);
    if (L.depth < 0) step<R>(G, L, out);
}

}  // namespace othx
