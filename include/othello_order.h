/*
 * othello_order.h — C-ABI of the ORDERED searches of libsubproc_amd_hip.so: the
 * depth-limited search (othello_search.h), search self-play (othello_play.h)
 * and the split search (othello_tree.h) with an `order` argument.  Conventions,
 * arguments, outputs and statuses are those headers'; only what `order` adds is
 * said here.
 *
 * The functions of this header are prefixed otho_ (the unordered sets othm_,
 * othp_ and otht_ are what they were).
 *
 * order == 0: exactly the unordered call (moves lowest square first; the same
 *             kernel).
 * order == 1: move ordering, the rule below (the *_ordered kernels).
 * anything else: OTH_EINVAL.
 *
 * THE RULE (order == 1).  A frame of the search with moves left picks
 *   1. a single move left: that move;
 *   2. with >= 2 moves left and >= 3 plies left below the frame (the root
 *      included), MOBILITY ORDER: the move that minimises the opponent's
 *      mobility after it, popcount(moves(child)), minus 3 when the move is a
 *      corner; ties to the lowest square.  The frame scores all its remaining
 *      moves again on every pick (nothing is stored per frame), one candidate
 *      per step of the lane's state machine;
 *   3. every other frame, STATIC CLASS ORDER: the lowest square of the first
 *      non-empty of the classes corners, A squares and their like (the eval's
 *      regions 0, 3, 4, 7, 6, 5 in that order), C squares (region 1), X squares
 *      (region 2).
 * ROOT TIE RULE.  The best move stays the LOWEST square among the maximisers:
 * a root move whose square is lower than the current best move's is searched
 * from alpha - 1 (its child's beta one wider), so a score of exactly alpha is
 * exact; it then takes over the best move, alpha unchanged.  Roots entered by a
 * pass and roots with no best move yet are unaffected.  Inside the split
 * search's tasks the rule is off: a task's root is an inner node of the tree,
 * whose expansion and slab order stay ascending.
 *
 * RESULTS.  value, best_move and status (and every byte of a game) equal the
 * order == 0 call's, ties included — EXCEPT for a position within reach of
 * node_limit: the two trees differ, so one order may end it as OTHM_LIMIT where
 * the other searches it.  With the default limit that needs a search of 2^28
 * nodes.
 *
 * NODES.  nodes counts every placement, the scoring placements of rule 2
 * included, plus passes; node_limit bounds that sum (a position that needs
 * exactly node_limit is searched, one more ends as OTHM_LIMIT), so the limit
 * alone still bounds a launch's run time.  The count is a function of the
 * position, the mover, the depth, the table, the order and the build only; it
 * differs between the orders and stays a diagnostic.
 */
#ifndef SUBPROC_AMD_OTHELLO_ORDER_H
#define SUBPROC_AMD_OTHELLO_ORDER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTHO_MAX_ORDER 1

/* othm_search with `order` */
int otho_search_ordered(const uint64_t* boards, const uint8_t* turn, int depth, int order, const int8_t* weights,
                        uint32_t node_limit, int32_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
                        uint64_t* work, int64_t n, void* stream);

/* othp_play with `order`: both players search with it; a game's moves do not
 * depend on it */
int otho_play_ordered(const uint64_t* start, const uint8_t* start_turn, uint64_t seed, uint64_t game_id0,
                      const int8_t* weights_a, const int8_t* weights_b, int depth_a, int depth_b, int exact_empties,
                      int order, int n_rand_a, int n_rand_b, int swap_colours, uint32_t node_limit, uint8_t* a_black,
                      uint64_t* final_boards, int8_t* diff, uint8_t* plies, uint8_t* moves, uint8_t* status,
                      uint64_t* nodes, int64_t* hist, uint64_t* work, int64_t n, void* stream);

/* otht_search with `order`: the searches inside the tasks are ordered (root tie
 * rule off), the tree's expansion is not; scratch as otht_scratch_bytes says */
int otho_tree_ordered(const uint64_t* boards, const uint8_t* turn, int depth, int split, int order,
                      const int8_t* weights, uint32_t node_limit, int32_t* value, uint8_t* best_move, uint8_t* status,
                      uint32_t* nodes, void* scratch, int64_t scratch_bytes, int32_t nodes_per_position,
                      uint64_t* work, int64_t n, void* stream);

/* blocks the launch uses at this order (no launch; cf. othm_search_grid,
 * othp_play_grid, otht_search_grid): the ordered kernels hold a few more
 * registers, so their resident count is asked for separately */
int otho_search_ordered_grid(int64_t n, int order);
int otho_play_ordered_grid(int64_t n, int order);
int otho_tree_ordered_grid(int64_t tasks, int order);

#ifdef __cplusplus
}
#endif
#endif
