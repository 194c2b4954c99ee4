// solve_order_core.hpp — solve_core.hpp's state machine with MOVE ORDERING: the
// same frames, Lane, pop() and settle_child(), a different choice of the next
// move.  Written once for the device (solve_tree.hip's ordered task kernel) and
// the host (tools/diag/solve_tree_host.cpp with order = 1).  The choice is made
// by order_core.hpp's pieces (§16), the very functions the search's ordered
// machine uses, with this file's size test for the mobility order.  DESIGN.md §17.
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
// THE SCORING STEP is order_core.hpp's: a step takes ONE candidate off the register-held
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
// the task started.  solve_core.hpp's pieces around order_core.hpp's head.
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
        othm::order_begin(Q, L.M, [&] { return 64 - R::count(L.P | L.O) >= kMobilityEmpties; });
        scoring = Q.cand != 0;
        sq = scoring ? othm::order_candidate<R>(Q) : othm::order_choice<R>(Q, L.M);
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
        return othm::order_keep(Q, (((u32)R::count(cm) + corner) << 6) | sq);
    }
    settle_child<R>(L, stk, limit, mv, X, Y, cm);
}

}  // namespace oths
