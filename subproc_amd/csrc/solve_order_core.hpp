// solve_order_core.hpp — solve_core.hpp's state machine with MOVE ORDERING: the
// same frames, Lane, start_task() and pop(), a different choice of the next
// move.  Written once for the device (solve_tree.hip's ordered task kernel) and
// the host (tools/diag/solve_tree_host.cpp with order = 1).  DESIGN.md §17;
// the search's twin is order_core.hpp (§16).
//
// THE RULE (the contract of `order = 1` inside a task).  A frame with moves
// left picks:
//   1. SINGLE MOVE.  One move left: it is played.
//   2. MOBILITY ORDER, for a frame with >= 2 moves left and at least
//      kMobilityEmpties empty squares: the move m that minimises
//          popcount(moves(child after m)) - (m is a corner ? 3 : 0),
//      ties to the lowest square.  The frame scores ALL its remaining moves
//      again on every pick, one candidate per step, so nothing is stored per
//      frame: the frames in LDS keep their 7 words.
//   3. STATIC CLASS ORDER, every other frame: order_core.hpp's static_pick().
// There is no root tie rule: a task's depth-0 frame is an inner tree node, and
// the tree's root reads its move off its children (solve_tree_core.hpp).
//
// THE SCORING STEP is §16's: a step takes ONE candidate off the register-held
// mask Order::cand, does one flips and one moves for it and keeps the running
// minimum in Order::pick as (score + 3) << 6 | square; the step that empties
// the mask leaves the chosen square in `pick`, the FOLLOWING step plays it.
//
// RESULTS.  apply_score takes strict improvements and cuts at alpha >= beta, so
// a frame returns its exact value inside its window and a bound outside it
// whatever the order: a task's report has the same fail-hard property under
// both orders.
//
// NODES = placements (scoring placements included) + passes; `limit` bounds
// that sum exactly as in the unordered machine.
#pragma once
#include <stdint.h>

#include "order_core.hpp"
#include "solve_core.hpp"

namespace oths {

// frames with at least this many empties (and >= 2 moves) order by mobility;
// chosen from the host build's exact node counts (the macro is
// for that comparison only: tools/diag/solve_tree_host.cpp -DOTHS_MOBILITY_EMPTIES=k)
#ifndef OTHS_MOBILITY_EMPTIES
#define OTHS_MOBILITY_EMPTIES 6
#endif
constexpr int kMobilityEmpties = OTHS_MOBILITY_EMPTIES;

// one step of the lane's ordered search; requires L.depth >= 0 and Q reset when
// the task started.  advance()'s twin: its pass, game-over and push code line
// for line (kept apart so that solve_kernel compiles from the text it always
// had), with the pick of the header.
template <class R, class S>
OTHS_FN void advance_ordered(Lane& L, othm::Order& Q, S& stk, u32 limit) {
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int r = 0; r < kPopsPerStep; r++)
        if (L.depth >= 0 && L.M == 0 && !(L.flags & (kFresh | kRootNew))) pop(L, stk);
    if (L.depth < 0) return;
    u64 X, Y;  // the position to analyse: X to move
    const bool mv = L.M != 0;
    bool scoring = false;
    u32 sq = 0;
    if (mv) {
        if (L.nodes >= limit) return stop_at_limit(L);
        if (Q.cand == 0 && Q.pick >= 64u && (L.M & (L.M - 1)) != 0 &&
            64 - R::count(L.P | L.O) >= kMobilityEmpties) {
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
            sq = othm::static_pick<R>(L.M);
        }
        const u64 bit = 1ull << sq;
        const u64 f = R::flips(sq, L.P, L.O);
        X = L.O & ~f;
        Y = L.P | f | bit;
        L.nodes++;
        if (!scoring) {
            Q.pick = othm::kPickNone;
            L.M &= ~bit;
            if (L.depth == 0) L.root_mv = sq;
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
        const u32 corner = (othm::kRegion0 >> sq) & 1u ? 0u : (u32)othm::kCornerBonus;
        const u32 key = (((u32)R::count(cm) + corner) << 6) | sq;
        if (key < Q.pick) Q.pick = key;
        if (Q.cand == 0) Q.pick &= 63u;  // chosen: the next step plays it
        return;
    }
    if (mv) {
        if (~(X | Y) == 0) {  // board full: the child's value for us, nothing pushed
            apply_score(L, R::count(Y) - R::count(X));
            return;
        }
        if (L.depth >= kFrames) return stop_at_limit(L);
        stk.store(L.depth, L.P, L.O, L.M, pack(L.alpha, L.beta, L.flags));
        L.depth++;
        L.P = X;
        L.O = Y;
        L.M = cm;
        const int a = L.alpha;
        L.alpha = -L.beta;
        L.beta = -a;
        L.flags = cm ? 0u : kFresh;
    } else if (L.flags & kRootNew) {
        L.M = cm;
        L.flags = cm ? 0u : kFresh;
    } else if (cm) {  // CHECK: a pass
        if (L.nodes >= limit) return stop_at_limit(L);
        L.nodes++;
        L.P = X;
        L.O = Y;
        L.M = cm;
        const int a = L.alpha;
        L.alpha = -L.beta;
        L.beta = -a;
        L.flags = kPassed;
        if (L.depth == 0) L.best_mv = kPassMove;
    } else {  // CHECK: game over; the next step pops the frame
        L.flags = 0;
        L.alpha = R::count(L.P) - R::count(L.O);
    }
}

}  // namespace oths
