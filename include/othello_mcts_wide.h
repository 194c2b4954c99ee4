/*
 * othello_mcts_wide.h — C-ABI of the wide Monte Carlo tree search of
 * libsubproc_amd_hip.so (subproc_amd/csrc/mcts_wide.hip, gfx950): othello_mcts.h's
 * search with several leaves per iteration, one block of waves per tree.
 * DESIGN.md §31.
 *
 * Conventions as in othello_mcts.h.  The functions of this header are prefixed
 * othv_ (othu_ is othello_mcts.h's set, othr_ othello_mcts_tree.h's).
 *
 * THE RULE.  Everything of othello_mcts.h holds: the node, the score, the tie
 * rules, the expansion test, the outputs, the statuses.  Only the iteration
 * changes.
 *
 * New argument: `leaves` L, 1..OTHV_MAX_LEAVES.  `iterations` R is now the
 * number of rounds; the tree gets N = R * L leaf visits.  The limits apply to
 * N: 1 <= N <= OTHU_MAX_ITERATIONS, so 128 * N stays exact in float32, and
 * log_table has N + 1 entries.
 *
 * One round r, for r = 0 .. R-1:
 *   A. WALKERS.  For walker w = 0 .. L-1, in this order:
 *      1. SELECT: step 1 of othello_mcts.h on the words as they stand now,
 *         the n that the earlier walkers of this round have added included.  A
 *         child with n == 0 is fresh; any other child is scored with its
 *         current n and s.
 *      2. EXPAND: step 2 unchanged, with n and the node count as they stand
 *         now.
 *      3. MARK: n += 1 on every node of the walker's path, root and leaf
 *         included.  s and d are not touched: until the back-up a pending
 *         visit counts as a loss for the side that moved into the node (a
 *         virtual loss), which pushes the later walkers away.
 *   B. PLAY OUT.  Walker w's 64 random games start from its leaf.  Lane j
 *      plays the game of global id game_id0 + ((i*R + r)*L + w)*64 + j (modulo
 *      2^64).  W and D as in step 3 of othello_mcts.h.
 *   C. BACK UP.  For every walker, from its leaf to the root: s += W, d += D,
 *      then (W, D) = (128 - W, -D) for the next node up.  n is counted already.
 *
 * Consequences.
 *   * With L = 1 every field equals othu_mcts with T = R: the walker's own
 *     marks come after its own selection, and the ids coincide.
 *   * Row i of a batch is the single call with game_id0 + i*R*L*64.
 *   * The answer depends on L.  It does not depend on the grid, the
 *     neighbouring positions or timing.
 *   * Several walkers of one round may end at the same leaf (a terminal root,
 *     a full tree, a forced line).  They play different games from it.
 *
 * How.  A block is L waves and owns one tree at a time, in slab blockIdx.x of
 * `scratch` (othello_mcts.h's node, OTHU_NODE_BYTES); trees are assigned to
 * blocks statically, grid-stride.  Wave 0 walks the L walkers one after
 * another while the other waves wait at the block's barrier; then wave w plays
 * walker w's 64 games and adds their sums along its path with vector atomics
 * on the slab (integer adds: any order gives the same words).  Two barriers a
 * round, each with a release/acquire fence at workgroup scope: the waves of a
 * block share a compute unit.  Nothing is ordered at agent scope, no wave spins
 * on memory and no block reads another block's slab.
 */
#ifndef SUBPROC_AMD_OTHELLO_MCTS_WIDE_H
#define SUBPROC_AMD_OTHELLO_MCTS_WIDE_H

#include <stdint.h>

#include "othello_mcts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OTHV_MAX_LEAVES 16   /* waves of a block: 1024 threads */
#define OTHV_MAX_BLOCKS 1024 /* the grid never exceeds this many blocks (slabs of scratch) */
#define OTHV_LDS_BYTES 14912 /* ray table 4096 + k-th bit table 2048 + 16 x (path 132 x 4 + leaf 16 + depth 4) */

/* Search the n positions boards[i] / turn[i]: othu_mcts's arguments, and
 *   iterations R >= 1, leaves L in 1..OTHV_MAX_LEAVES, R * L in
 *              1..OTHU_MAX_ITERATIONS, else OTH_EINVAL
 *   log_table  float32[R * L + 1], used as given
 *   scratch    scratch_bytes >= othv_mcts_wide_scratch_bytes(n, max_nodes, leaves)
 * OTH_MCTS_WIDE_BLOCKS in the environment (read per launch) caps the grid;
 * results do not depend on it. */
int othv_mcts_wide(const uint64_t* boards, const uint8_t* turn, int iterations, int leaves, float explore,
                   const float* log_table, uint64_t seed, uint64_t game_id0, int max_nodes, uint32_t* visits,
                   uint32_t* wins, int32_t* diffs, uint32_t* root_wins, int32_t* root_diffs, uint8_t* best_move,
                   uint8_t* status, uint32_t* nodes, void* scratch, int64_t scratch_bytes, int64_t n, void* stream);

/* bytes of scratch: min(n, OTHV_MAX_BLOCKS) slabs of OTHU_NODE_BYTES * max_nodes
 * (at least 16; OTH_EINVAL for n < 0, max_nodes outside 1..OTHU_MAX_NODES or
 * leaves outside 1..OTHV_MAX_LEAVES) */
int64_t othv_mcts_wide_scratch_bytes(int64_t n, int max_nodes, int leaves);

/* blocks of `leaves` waves a call on n positions launches (no launch): the
 * device's resident blocks under OTH_MCTS_WIDE_BLOCKS and OTHV_MAX_BLOCKS, at
 * most n; OTH_EINVAL for n < 0 or leaves outside 1..OTHV_MAX_LEAVES */
int othv_mcts_wide_grid(int64_t n, int leaves);

#ifdef __cplusplus
}
#endif
#endif
