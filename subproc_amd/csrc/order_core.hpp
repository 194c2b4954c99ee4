// order_core.hpp — search_core.hpp's state machine with MOVE ORDERING: the same
// frames, Lane, start(), pop() and eval(), a different choice of the next move.
// Written once for the device (search.hip, play.hip, tree.hip: the *_ordered
// kernels) and the host (tools/diag/*_host.cpp with order = 1).  DESIGN.md §16.
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

// a finished ROOT child's value with the root tie rule; other frames: apply_score
template <bool kRootTie>
OTHM_FN void apply_score_ordered(Lane& L, int score) {
    if (kRootTie && L.depth == 0 && score == L.alpha && L.root_mv < L.best_mv && L.best_mv < 64u)
        L.best_mv = L.root_mv;  // (the move was searched from alpha - 1: the score is exact)
    apply_score(L, score);
}

template <bool kRootTie, class S>
OTHM_FN void pop_ordered(Lane& L, S& stk) {
    const int score = (L.flags & kPassed) ? L.alpha : -L.alpha;  // for the parent's mover
    if (L.depth == 0) {
        L.depth = -1;
        L.value = -score;
        return;
    }
    L.depth--;
    u32 w;
    stk.load(L.depth, L.P, L.O, L.M, L.alpha, L.beta, w);
    L.flags = w & 0xFFu;
    L.rem = (int)(w >> 8);
    apply_score_ordered<kRootTie>(L, score);
}

// one step of the lane's ordered search; requires L.depth >= 0 and Q reset when
// the position started.  advance()'s twin: its leaf, pass, game-over and push
// code line for line (kept apart so that the unordered kernels compile from
// the text they always had), with the pick of the header.
template <class R, bool kRootTie, class S>
OTHM_FN void advance_ordered(Lane& L, Order& Q, S& stk, const int* table, u32 limit) {
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int r = 0; r < kPopsPerStep; r++)
        if (L.depth >= 0 && L.M == 0 && !(L.flags & (kFresh | kRootNew))) pop_ordered<kRootTie>(L, stk);
    if (L.depth < 0) return;
    u64 X, Y;  // the position to analyse: X to move
    const bool mv = L.M != 0;
    bool scoring = false;
    u32 sq = 0;
    int lower = 0;  // 1: a root move below the best move, searched from alpha - 1
    if (mv) {
        if (L.nodes >= limit) return stop_at_limit(L);
        if (Q.cand == 0 && Q.pick >= 64u && (L.M & (L.M - 1)) != 0 && L.rem >= kMobilityRem) {
            Q.cand = L.M;  // begin a pick: this step scores its first candidate
            Q.pick = ~0u;
        }
        scoring = Q.cand != 0;
        if (scoring) {
            sq = R::lowest(Q.cand);
            Q.cand &= Q.cand - 1;
        } else if (Q.pick < 64u) {
            sq = Q.pick;
        } else if ((L.M & (L.M - 1)) == 0) {
            sq = R::lowest(L.M);
        } else {
            sq = static_pick<R>(L.M);
        }
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
        const u32 key = (((u32)R::count(cm) + corner) << 6) | sq;
        if (key < Q.pick) Q.pick = key;
        if (Q.cand == 0) Q.pick &= 63u;  // chosen: the next step plays it
        return;
    }
    const u32 side = L.flags & kRootSide;
    if (mv) {
        if (L.rem <= 1 || ~(X | Y) == 0) {  // a leaf: scored here, nothing pushed
            u64 om = 0;
            if (side || cm == 0) om = R::moves(Y, X);
            int score;
            if ((cm | om) == 0) {
                score = kTerminal * (R::count(Y) - R::count(X));
            } else {
                const int e = eval<R>(table, side ? Y : X, side ? om : cm, (u32)R::count(X | Y));
                score = side ? e : -e;
            }
            apply_score_ordered<kRootTie>(L, score);  // (a leaf's score is exact: no window to widen)
            return;
        }
        if (L.depth >= kFrames) return stop_at_limit(L);
        stk.store(L.depth, L.P, L.O, L.M, L.alpha, L.beta, L.flags | ((u32)L.rem << 8));
        L.depth++;
        L.rem--;
        L.P = X;
        L.O = Y;
        L.M = cm;
        const int a = L.alpha - lower;
        L.alpha = -L.beta;
        L.beta = -a;
        L.flags = (cm ? 0u : kFresh) | (side ^ kRootSide);
    } else if (L.flags & kRootNew) {
        L.M = cm;
        L.flags = (cm ? 0u : kFresh) | kRootSide;
    } else if (cm) {  // CHECK: a pass (no depth spent)
        if (L.nodes >= limit) return stop_at_limit(L);
        L.nodes++;
        L.P = X;
        L.O = Y;
        L.M = cm;
        const int a = L.alpha;
        L.alpha = -L.beta;
        L.beta = -a;
        L.flags = kPassed | (side ^ kRootSide);
        if (L.depth == 0) L.best_mv = kPassMove;
    } else {  // CHECK: game over; the next step pops the frame
        L.flags = side;
        L.alpha = kTerminal * (R::count(L.P) - R::count(L.O));
    }
}

}  // namespace othm
