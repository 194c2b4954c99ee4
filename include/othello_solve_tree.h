/*
 * othello_solve_tree.h — C-ABI of the split endgame solver of
 * libsubproc_amd_hip.so (subproc_amd/csrc/solve_tree.hip, gfx950):
 * othello_solve.h's exact solve with each position's tree spread over the
 * whole device, for small batches (down to one position) and for up to
 * OTHE_MAX_EMPTIES empty squares.
 *
 * Conventions as in othello_solve.h: boards are 2 x uint64 [black, white] per
 * position, every pointer is DEVICE memory owned by the caller, calls are
 * asynchronous on `stream`, allocate nothing, never synchronise, and return
 * OTH_OK, OTH_EINVAL or -(hipError_t).
 *
 * The functions of this header are prefixed othe_ (oth_, oths_, othm_, othp_,
 * otht_ and otho_ are the other headers' sets).
 *
 * How.  The top of each position's tree is expanded into the position's slab
 * of `scratch`, level by level, until every node has at most `task_empties`
 * empty squares (a pass is a level of its own; the root is always expanded one
 * level when its mover has a move or must pass).  Every node at the bottom of
 * that tree becomes a task: an exact solve by oths_solve's one-lane state
 * machine (order 0) or by its ordered twin (order 1).  The tasks of all
 * positions are spread over the device's lanes and share alpha-beta bounds
 * through the tree.
 *
 * Value, best move: exactly othello_solve.h's.  value[i] = V(pos_i, mover) by
 * its three rules, the last of which is the project's result rule (the plain
 * disc difference, NO bonus for empty squares); best_move the LOWEST square
 * among the maximisers, 64 (OTH_PASS) for a forced pass at the root,
 * OTHS_NO_MOVE when the game is over at the root.
 * Status: OTHS_SKIPPED (more than max_empties empties: value 0, move 255,
 * nodes 0), OTHS_SOLVED, OTHS_INVALID (black & white overlap: value 0, move
 * 255, nodes 0) and OTHS_LIMIT as there, and OTHE_NOROOM.
 * A position's value, move and status are functions of the position, the
 * mover, max_empties, task_empties, node_limit and nodes_per_position, and of
 * `order` only within reach of node_limit; not of n, the neighbours, the grid,
 * the environment or the order in which tasks run.  One exception, inherent in
 * sharing bounds: how many nodes a task needs depends on the bounds it starts
 * with, so a position with a task within reach of node_limit may end as
 * OTHS_LIMIT in one run and as OTHS_SOLVED (with the right value) in another.
 *
 * order = 1 (subproc_amd/csrc/solve_order_core.hpp): inside a task a frame
 * with one move plays it; a frame with at least two moves and at least 6
 * empty squares plays the move that leaves the opponent the fewest moves
 * (corner moves count 3 less, ties to the lowest square); every other frame
 * takes othello_order.h's static class order.  The expansion is the same in
 * both orders.  Same values, moves and statuses from a smaller tree.
 */
#ifndef SUBPROC_AMD_OTHELLO_SOLVE_TREE_H
#define SUBPROC_AMD_OTHELLO_SOLVE_TREE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTHE_MAX_EMPTIES 16 /* OTHS_MAX_EMPTIES + 4 */
#define OTHE_NOROOM 4       /* status: the tree did not fit the position's slab and a task would have more than OTHS_MAX_EMPTIES empties */
#define OTHE_MIN_NODES 64   /* nodes_per_position's lower bound: the root's children always fit */

/* Solve the n positions boards[i] / turn[i] that have at most max_empties
 * empty squares.  0 <= max_empties <= OTHE_MAX_EMPTIES, 1 <= task_empties <=
 * OTHS_MAX_EMPTIES and order in {0, 1}, else OTH_EINVAL.
 *   value     int8[n]   V from the mover's side
 *   best_move uint8[n]
 *   status    uint8[n]  OTHS_SKIPPED / SOLVED / INVALID / LIMIT, OTHE_NOROOM
 *   nodes     uint32[n] the expansion's nodes plus the tasks' placements
 *             (with order 1 the scoring placements too) and passes,
 *             saturating.  The tasks' windows depend on when they start, so
 *             this count DEPENDS ON TIMING: a diagnostic, nothing may compare it.
 * Each of the four may be NULL.
 *   node_limit  bounds EVERY TASK's search (0 = OTHS_DEFAULT_NODE_LIMIT),
 *               which bounds the kernel's run time; a position with any task
 *               at the limit ends as OTHS_LIMIT with value 0 and move 255
 *   scratch     scratch_bytes >= othe_scratch_bytes(n, nodes_per_position) of
 *               device memory, 8-byte aligned, contents irrelevant before and
 *               after; it must not be shared with a launch that may overlap
 *   nodes_per_position  >= OTHE_MIN_NODES: the slab of each position's tree.  A
 *               level is expanded whole or not at all; when the next level does
 *               not fit, the tasks start higher and search deeper.  If one would
 *               then have more than OTHS_MAX_EMPTIES empties, the position ends
 *               as OTHE_NOROOM with value 0 and move 255: a function of the
 *               position, task_empties and nodes_per_position only.
 *   work        one device word, 0 at launch, left at 0 (oth_rollout's
 *               contract); may be shared with rollouts, solves, searches and
 *               plays on the same stream
 * n == 0: OTH_OK, nothing launched.  OTH_SOLVE_BLOCKS in the environment (read
 * per launch) caps the task kernel's grid as it does oths_solve's; results do
 * not depend on it. */
int othe_solve(const uint64_t* boards, const uint8_t* turn, int max_empties, int task_empties, int order,
               uint32_t node_limit, int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
               void* scratch, int64_t scratch_bytes, int32_t nodes_per_position, uint64_t* work, int64_t n,
               void* stream);

/* bytes of scratch a call with these arguments needs (OTH_EINVAL for n < 0,
 * nodes_per_position < OTHE_MIN_NODES or a size beyond 2^55 nodes) */
int64_t othe_scratch_bytes(int64_t n, int32_t nodes_per_position);

/* blocks the task kernel launches for this many tasks (no launch; cf.
 * oths_solve_grid) */
int othe_solve_grid(int64_t tasks);

#ifdef __cplusplus
}
#endif
#endif
