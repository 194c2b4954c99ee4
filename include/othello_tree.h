/*
 * othello_tree.h — C-ABI of the split search of libsubproc_amd_hip.so
 * (subproc_amd/csrc/tree.hip, gfx950): othello_search.h's depth-limited search
 * with each position's tree spread over the whole device, for small batches
 * (down to one position) and for depths beyond OTHM_MAX_DEPTH.
 *
 * Conventions as in othello_search.h: boards are 2 x uint64 [black, white] per
 * position, every pointer is DEVICE memory owned by the caller EXCEPT `weights`
 * (host), calls are asynchronous on `stream`, allocate nothing, never
 * synchronise, and return OTH_OK, OTH_EINVAL or -(hipError_t).
 *
 * The functions of this header are prefixed otht_ (oth_, oths_, othm_ and othp_
 * are the other headers' sets).
 *
 * How.  The top `split` plies of each position are expanded into a tree in the
 * position's slab of `scratch` (a pass costs no depth there either, so a slab
 * may hold up to 2 * split + 1 levels).  Every node at the bottom of that tree
 * becomes a task: a search of the remaining depth - split plies by
 * othm_search's one-lane state machine.  The tasks of all positions are spread
 * over the device's lanes and share alpha-beta bounds through the tree
 * (DESIGN.md §15).
 *
 * Value, best move: exactly othello_search.h's.  value[i] = S(pos_i, r, depth)
 * by its four rules, best_move the LOWEST square among the maximisers, 64 for a
 * forced pass at the root, OTHM_NO_MOVE when the game is over at the root.
 * Status: OTHM_SEARCHED, OTHM_INVALID and OTHM_LIMIT as there, and OTHT_NOROOM.
 * A position's value, move and status are functions of the position, the mover,
 * depth, split, the table, node_limit and nodes_per_position; not of n, the
 * neighbours, the grid, the environment or the order in which tasks run.  One
 * exception, inherent in sharing bounds: how many nodes a task needs depends on
 * the bounds it starts with, so a position with a task within reach of
 * node_limit may end as OTHM_LIMIT in one run and as OTHM_SEARCHED (with the
 * right value) in another.
 */
#ifndef SUBPROC_AMD_OTHELLO_TREE_H
#define SUBPROC_AMD_OTHELLO_TREE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTHT_MAX_SPLIT 4
#define OTHT_NOROOM 4    /* status: the split tree did not fit the position's slab and the frontier is deeper than 8 plies */
#define OTHT_MIN_NODES 64 /* nodes_per_position's lower bound: the root's children always fit */

/* Search the n positions boards[i] / turn[i] to `depth` plies, the top `split`
 * of them in the tree: 1 <= split <= OTHT_MAX_SPLIT and split < depth <= split +
 * OTHM_MAX_DEPTH, else OTH_EINVAL.
 *   weights, value, best_move, status: as othm_search's (each output may be NULL)
 *   node_limit  bounds EVERY TASK's search (0 = OTHM_DEFAULT_NODE_LIMIT), which
 *               bounds the kernel's run time; a position with any task at the
 *               limit ends as OTHM_LIMIT with value 0 and move 255
 *   nodes       uint32[n] the expansion's nodes plus the tasks', saturating.
 *               The tasks' windows depend on when they start, so this count
 *               DEPENDS ON TIMING: a diagnostic, nothing may compare it.
 *   scratch     scratch_bytes >= otht_scratch_bytes(n, nodes_per_position) of
 *               device memory, 8-byte aligned, contents irrelevant before and
 *               after; it must not be shared with a launch that may overlap
 *   nodes_per_position  >= OTHT_MIN_NODES: the slab of each position's tree.  A
 *               level is expanded whole or not at all; when the next level does
 *               not fit, the tasks start higher and search deeper.  If one would
 *               then have more than OTHM_MAX_DEPTH plies left, the position ends
 *               as OTHT_NOROOM with value 0 and move 255.
 *   work        one device word, 0 at launch, left at 0 (oth_rollout's
 *               contract); may be shared with rollouts, solves, searches and
 *               plays on the same stream
 * n == 0: OTH_OK, nothing launched.  OTH_SEARCH_BLOCKS in the environment caps
 * the task kernel's grid as it does othm_search's; results do not depend on it. */
int otht_search(const uint64_t* boards, const uint8_t* turn, int depth, int split, const int8_t* weights,
                uint32_t node_limit, int32_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
                void* scratch, int64_t scratch_bytes, int32_t nodes_per_position, uint64_t* work, int64_t n,
                void* stream);

/* bytes of scratch a call with these arguments needs (OTH_EINVAL for n < 0,
 * nodes_per_position < OTHT_MIN_NODES or a size beyond 2^55 nodes) */
int64_t otht_scratch_bytes(int64_t n, int32_t nodes_per_position);

/* blocks the task kernel launches for this many tasks (no launch; cf.
 * othm_search_grid) */
int otht_search_grid(int64_t tasks);

#ifdef __cplusplus
}
#endif
#endif
