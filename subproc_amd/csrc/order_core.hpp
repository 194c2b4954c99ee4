// order_core.hpp — search_core.hpp's state machine with MOVE ORDERING: the same
// frames, Lane, start(), pop(), settle_child() and eval(), a different choice of
// the next move.  Written once for the device (search.hip, play.hip, tree.hip:
// the *_ordered kernels) and the host (tools/diag/*_host.cpp with order = 1).
// The choice itself (the Order state and its pieces below) is the solver's too:
// solve_order_core.hpp puts it in front of solve_core.hpp's transitions.
// DESIGN.md §16.
//
// THE RULE (the contract of `order = 1`).  A frame with moves left picks:
//   1. SINGLE MOVE.  One move left: it is played.
//   2. MOBILITY ORDER, for a frame with >= 2 moves left and rem >= kMobilityRem
//      (3), the root included: the move m that minimises
//          popcount(moves(child after m)) - (m is a corner ? kCornerBonus : 0),
//      kCornerBonus = 3, ties to the lowest square.  The frame scores ALL its
//      remaining moves again on every pick, one candidate per step (below), so
//      nothing is stored per frame: the frames in LDS keep their 9 words.
//   3. STATIC CLASS ORDER, every other frame: the lowest square of the first
//      non-empty class of kRegion0 (corners), 3, 4, 7, 6, 5, kRegion1 (C
//      squares), kRegion2 (X squares).
//
// THE SCORING STEP.  A lane must not loop over its candidates while the other
// 63 wait, so scoring is one more transition of the machine: a step takes ONE
// candidate off the register-held mask Order::cand, does one flips and one
// moves for it (a node step's instruction mix) and keeps the running minimum
// in Order::pick as (score + kCornerBonus) << 6 | square.  The step that
// empties the mask leaves the chosen square in `pick`; the FOLLOWING step plays
// it.  Only the current frame scores: a push happens only from a step that
// plays, when the scoring state is idle again.
//
// RESULTS.  Below the root the order cannot change a result: apply_score takes
// strict improvements and cuts at alpha >= beta, so a frame returns its exact
// value inside its window and a bound outside it whatever the order.  AT the
// root the unordered search's best move is the LOWEST square among the
// maximisers, which ascending order gives for free.  The ROOT TIE RULE keeps
// it (template parameter kRootTie, on for searches and games, off for the split
// search's tasks, whose depth-0 frame is an inner tree node): a root move whose
// square is lower than the current best move's is searched with its child's
// beta widened by one (the child's window comes from alpha - 1), so a score of
// exactly alpha is exact, not a bound; it then takes over best_mv without
// changing alpha.  Roots entered by a pass (best_mv = 64) and roots without a
// best move yet are unaffected.  So value, best move and status equal the
// unordered search's on every position — EXCEPT within reach of the node
// limit: the trees differ, so a position may end as kLimit under one order and
// be searched under the other.
//
// NODES.  nodes = placements (scoring placements included) + passes;
// `limit` bounds that sum exactly as in the unordered machine (a step that
// would count node limit + 1 ends the position as kLimit), so a launch's run
// time stays bounded by the limit alone.  It is a function of the position,
// the mover, the depth, the table, the order and the build only.
#pragma once
#include <stdint.h>

#include "search_core.hpp"

namespace othm {

constexpr int kMobilityRem = 3;   // frames with rem >= this (and >= 2 moves) order by mobility
constexpr int kCornerBonus = 3;   // taken off a corner move's score
constexpr u32 kPickNone = 255;    // Order::pick: nothing chosen

// the scoring state of the lane's CURRENT frame, in registers
//   idle:    cand == 0, pick == kPickNone
//   scoring: cand != 0, pick = the running minimum key (~0u before the first)
//   chosen:  cand == 0, pick < 64: the square the next step plays
struct Order {
    u64 cand;
    u32 pick;
};

OTHM_FN void order_reset(Order& Q) {
    Q.cand = 0;
    Q.pick = kPickNone;
}

// rule 3's square: m != 0
template <class R>
OTHM_FN u32 static_pick(u64 m) {
    u64 c = m & kRegion2;
    if (m & kRegion1) c = m & kRegion1;
    if (m & kRegion5) c = m & kRegion5;
    if (m & kRegion6) c = m & kRegion6;
    if (m & kRegion7) c = m & kRegion7;
    if (m & kRegion4) c = m & kRegion4;
    if (m & kRegion3) c = m & kRegion3;
    if (m & kRegion0) c = m & kRegion0;
    return R::lowest(c);
}

// THE HEAD, shared with the solver's ordered machine (solve_order_core.hpp),
// in three pieces.  A step with moves left calls order_begin(); then Q.cand != 0
// says that it SCORES: it places order_candidate()'s square and hands the
// child's moves to order_score(); otherwise it PLAYS order_choice()'s square.

// begin a pick where rule 2 applies: `mobile()` is its size test, asked only of
// a frame with >= 2 moves left and no pick under way
template <class Mobile>
OTHM_FN void order_begin(Order& Q, u64 M, Mobile mobile) {
    if (Q.cand == 0 && Q.pick >= 64u && (M & (M - 1)) != 0 && mobile()) {
        Q.cand = M;  // this step scores its first candidate
        Q.pick = ~0u;
    }
}

// take the next candidate off the mask
template <class R>
OTHM_FN u32 order_candidate(Order& Q) {
    const u32 sq = R::lowest(Q.cand);
    Q.cand &= Q.cand - 1;
    return sq;
}

// the square to play: the pick just chosen, the single move, or rule 3's
template <class R>
OTHM_FN u32 order_choice(const Order& Q, u64 M) {
    if (Q.pick < 64u) return Q.pick;
    if ((M & (M - 1)) == 0) return R::lowest(M);
    return static_pick<R>(M);
}

// THE SCORING STEP's end: the candidate's key against the running minimum
OTHM_FN void order_keep(Order& Q, u32 key) {
    if (key < Q.pick) Q.pick = key;
    if (Q.cand == 0) Q.pick &= 63u;  // chosen: the next step plays it
}

// one step of the lane's ordered search; requires L.depth >= 0 and Q reset when
// the position started.  search_core.hpp's pieces around the head above.
template <class R, bool kRootTie, class S>
OTHM_FN void advance_ordered(Lane& L, Order& Q, S& stk, const int* table, u32 limit) {
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int r = 0; r < kPopsPerStep; r++)
        if (L.depth >= 0 && L.M == 0 && !(L.flags & (kFresh | kRootNew))) pop<kRootTie>(L, stk);
    if (L.depth < 0) return;
    u64 X, Y;  // the position to analyse: X to move
    const bool mv = L.M != 0;
    bool scoring = false;
    u32 sq = 0;
    int lower = 0;  // 1: a root move below the best move, searched from alpha - 1
    if (mv) {
        if (L.nodes >= limit) return stop_at_limit(L);
        order_begin(Q, L.M, [&] { return L.rem >= kMobilityRem; });
        scoring = Q.cand != 0;
        sq = scoring ? order_candidate<R>(Q) : order_choice<R>(Q, L.M);
        const u64 bit = 1ull << sq;
        const u64 f = R::flips(sq, L.P, L.O);
        X = L.O & ~f;
        Y = L.P | f | bit;
        L.nodes++;
        if (!scoring) {
            Q.pick = kPickNone;
            L.M &= ~bit;
            if (L.depth == 0) {
                L.root_mv = sq;
                if (kRootTie && sq < L.best_mv && L.best_mv < 64u) lower = 1;
            }
        }
    } else if (L.flags & kRootNew) {
        X = L.P;
        Y = L.O;
    } else if (L.flags & kFresh) {
        X = L.O;
        Y = L.P;
    } else {
        return;  // a third finished frame in a row: the next step pops it
    }
    const u64 cm = R::moves(X, Y);
    if (scoring) {
        const u32 corner = (kRegion0 >> sq) & 1u ? 0u : (u32)kCornerBonus;
        return order_keep(Q, (((u32)R::count(cm) + corner) << 6) | sq);
    }
    settle_child<R, kRootTie>(L, stk, table, limit, mv, X, Y, cm, lower);
}

}  // namespace othm
