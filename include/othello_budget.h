/*
 * othello_budget.h — C-ABI of the searches by NODE BUDGET of
 * libsubproc_amd_hip.so (subproc_amd/csrc/budget.hip, gfx950): iterative
 * deepening with othello_search.h's search, for a batch of positions and inside
 * othello_play.h's games.  Conventions as in othello_search.h: boards are
 * 2 x uint64 [black, white], every pointer is DEVICE memory owned by the caller
 * EXCEPT the weight tables (host), calls are asynchronous on `stream`, allocate
 * nothing, never synchronise, and return OTH_OK, OTH_EINVAL or -(hipError_t).
 *
 * The functions of this header are prefixed othb_ (othm_ is the fixed-depth
 * search's set, othp_ the games', otho_ the ordered calls').
 *
 * THE RULE.  Position i is searched for its root mover (othm_search's rule) with
 * the eval table W, a budget B_i >= 1 (nodes) and a depth cap D in
 * 1..OTHM_MAX_DEPTH.
 *   1. Let E be the position's empty squares and K = min(D, max(1, E)): a pass
 *      costs no depth, so depth E already searches the whole tree
 *      (othello_search.h, "Value").
 *   2. rem_1 = B_i.
 *   3. For d = 1..K, iteration d is exactly othm_search's search of the position
 *      at depth d (otho_search_ordered's with order == 1): the same machine,
 *      move order, window, tie rule and node count, with node limit rem_d.
 *   4. An iteration that needs more than rem_d nodes ends the loop; one that
 *      needs exactly rem_d completes.
 *   5. A completed iteration of n_d nodes records its value, best move and d,
 *      and rem_{d+1} = rem_d - n_d.  The loop also ends when rem_{d+1} == 0.
 * Outputs: value and best_move of the deepest completed iteration; depth[i] that
 * iteration's d; status OTHM_SEARCHED, or OTHM_LIMIT when not even depth 1
 * completed (value 0, best_move 255, depth 0, nodes 0); overlapping boards give
 * OTHM_INVALID (value 0, best_move 255, depth 0, nodes 0).  nodes[i] is the sum
 * of the completed iterations' n_d, so it never exceeds B_i.
 *
 * The results are a function of the position, the mover, the table, B_i, D,
 * `order` and the build only: not of n, the neighbours or the grid.
 *
 * Iterations share nothing: no move of the previous iteration is tried first and
 * there is no aspiration window, so every field can be checked against
 * othm_search depth by depth.  With order == 1 the values and moves per depth
 * are the same (othello_order.h, "Results"), n_d is the ordered search's count,
 * so the depth reached may differ.
 *
 * One GPU lane per position or game; a lane's work is bounded by its budget
 * (DESIGN.md §22).
 */
#ifndef SUBPROC_AMD_OTHELLO_BUDGET_H
#define SUBPROC_AMD_OTHELLO_BUDGET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Search the n positions boards[i] / turn[i] by budget.
 *   max_depth  the cap D, 1..OTHM_MAX_DEPTH, else OTH_EINVAL
 *   weights    HOST int8[36], as othm_search's (NULL: OTH_EINVAL)
 *   budget     every position's budget when budgets == NULL; then 0 is OTH_EINVAL
 *   budgets    uint32[n] or NULL: each position's budget; a position whose
 *              budget is 0 ends as OTHM_LIMIT
 *   order      0 or 1 (othello_order.h), else OTH_EINVAL
 *   value      int32[n]
 *   best_move  uint8[n]
 *   depth      uint8[n]  the deepest completed iteration, 0: none
 *   status     uint8[n]  OTHM_SEARCHED / INVALID / LIMIT
 *   nodes      uint32[n] the completed iterations' nodes
 * Each of the five may be NULL.  work: one device word, 0 at launch, left at 0:
 * othm_search's contract, and a stream's launches may share the word with it.
 * n == 0: OTH_OK, nothing launched.
 * OTH_BUDGET_BLOCKS in the environment (read per launch) caps the grid of both
 * calls, from 1 to the resident count; results do not depend on it. */
int othb_search(const uint64_t* boards, const uint8_t* turn, int max_depth, const int8_t* weights, uint32_t budget,
                const uint32_t* budgets, int order, int32_t* value, uint8_t* best_move, uint8_t* depth,
                uint8_t* status, uint32_t* nodes, uint64_t* work, int64_t n, void* stream);

/* othp_play (othello_play.h: the games, the draws, the outputs, the statuses)
 * with rule 4 of its turn changed: the move is othb_search's best_move for the
 * position and the mover with the mover's table, budget (budget_a / budget_b,
 * >= 1, else OTH_EINVAL) and depth cap (depth_a / depth_b).  A position whose
 * depth 1 does not complete stops the game as OTHM_LIMIT.  exact_empties keeps
 * its meaning: once a position has empties <= exact_empties, its move comes from
 * ONE search of max(cap, empties) plies under node_limit, without a budget.
 * nodes[i] sums the completed iterations of the game's budget searches and the
 * nodes of its searches without a budget.  order as otho_play_ordered's. */
int othb_play(const uint64_t* start, const uint8_t* start_turn, uint64_t seed, uint64_t game_id0,
              const int8_t* weights_a, const int8_t* weights_b, int depth_a, int depth_b, uint32_t budget_a,
              uint32_t budget_b, int exact_empties, int order, int n_rand_a, int n_rand_b, int swap_colours,
              uint32_t node_limit, uint8_t* a_black, uint64_t* final_boards, int8_t* diff, uint8_t* plies,
              uint8_t* moves, uint8_t* status, uint64_t* nodes, int64_t* hist, uint64_t* work, int64_t n,
              void* stream);

/* blocks a launch of n positions / games uses at order 0 (no launch; cf.
 * othm_search_grid) */
int othb_search_grid(int64_t n);
int othb_play_grid(int64_t n);

#ifdef __cplusplus
}
#endif
#endif
