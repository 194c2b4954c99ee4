/*
 * othello_mcts.h — C-ABI of the Monte Carlo tree search of
 * libsubproc_amd_hip.so (subproc_amd/csrc/mcts.hip, gfx950): UCT over uniform
 * random playouts, one tree per position, one wave per tree.  DESIGN.md §28.
 *
 * Conventions as in othello_solve.h: boards are 2 x uint64 [black, white] per
 * position, every pointer is DEVICE memory owned by the caller, calls are
 * asynchronous on `stream`, allocate nothing, never synchronise, and return
 * OTH_OK, OTH_EINVAL or -(hipError_t).
 *
 * The functions of this header are prefixed othu_ (oth_, oths_, othm_, othp_,
 * otht_, otho_, othe_, othh_, othw_, otha_, othb_, othl_, othx_ and othc_ are
 * the other headers' sets).
 *
 * THE RULE.  Everything is integer except the selection score, which is
 * float32 built from individually rounded operations (no contraction into a
 * fused multiply-add; `/` and sqrt correctly rounded).  The outputs are a
 * function of the inputs only: not of the grid, the neighbouring positions or
 * timing.
 *
 * Inputs.  Position i has a board, a mover (turn[i] == 2: White, anything
 * else, or turn == NULL: Black), `iterations` T, the exploration constant
 * `explore` c (float32), `seed`, `game_id0`, `max_nodes` M and the table
 * log_table[0..T] of float32.
 *
 * Node.  A node holds the mover's discs P, the other side's discs O, visits
 * n, half-points s, disc sum d, and its children as a contiguous index range
 * [first, first + cnt).  Nodes are numbered in creation order; node 0 is the
 * root.  A node's mover is the opponent of its parent's mover, across a pass
 * edge too.  s and d are kept from the point of view of the side that moved
 * INTO the node: the opponent of the node's mover.
 *
 * One iteration t, for t = 0 .. T-1:
 *   1. SELECT.  v = 0.  While v is expanded, move to a child: the first child
 *      in index order with n == 0 if there is one, otherwise the child c that
 *      maximises, in float32,
 *          mean  = float(s_c) / float(128 * n_c)
 *          score = mean + c * sqrt(log_table[n_v] / float(n_c))
 *      under a strict `>`: ties go to the lowest index.
 *   2. EXPAND, only if v is not terminal (a node is terminal when neither side
 *      can move), v is the root or v.n > 0, and nodes + cnt <= M, where cnt is
 *      the number of legal moves of v's mover, 1 for a forced pass.  The
 *      children are appended in ascending square order (a pass child is the
 *      same discs with the mover swapped), v is marked expanded and the walk
 *      goes to the first child.  Otherwise it stays at v.
 *   3. PLAY OUT 64 uniformly random games from the leaf.  Lane j plays the
 *      game of global id game_id0 + (i*T + t)*64 + j (modulo 2^64) of `seed`
 *      (DESIGN.md §4's key and draws: what oth_rollout plays from `start` =
 *      the leaf for that id).  With dp the final disc difference from the
 *      point of view of the OPPONENT of the leaf's mover,
 *          W = sum of (2 if dp > 0, 1 if dp == 0, 0 otherwise),  D = sum of dp.
 *      A terminal leaf needs no special case: its 64 games end at once.
 *   4. BACK UP from the leaf to the root: n += 1, s += W, d += D, then
 *      (W, D) = (128 - W, -D) for the next node up.
 *
 * Outputs, per position i (each pointer may be NULL):
 *   visits[i*64+sq] (uint32), wins[i*64+sq] (uint32), diffs[i*64+sq] (int32)
 *                  n, s and d of the root child reached by square sq (already
 *                  from the root mover's side); 0 elsewhere
 *   root_wins[i]   (uint32) 128 * n_root - s_root
 *   root_diffs[i]  (int32)  -d_root
 *   best_move[i]   the root move with the most visits, ties to more wins, then
 *                  to the lowest square; OTH_PASS where the root must pass,
 *                  255 where the game is over at the root
 *   nodes[i]       (uint32) nodes created, the root included: deterministic
 *   status[i]      OTHU_SEARCHED, or OTHU_INVALID: black & white overlap, every
 *                  other field 0 and best_move 255
 *
 * Limits.  1 <= T <= OTHU_MAX_ITERATIONS = 65,536: 128*T = 2^23 is exact in
 * float32 and |d| <= 4096*T fits int32.  1 <= M <= OTHU_MAX_NODES = 2^20.
 *
 * How.  A block is one wave and owns one tree at a time; trees are assigned to
 * blocks statically, grid-stride (block b walks positions b, b + grid, ...), and
 * block b keeps its tree in slab b of `scratch` (OTHU_NODE_BYTES per node).
 * The wave's 64 lanes are the 64 playouts of an iteration and, in selection
 * and expansion, the children of a node.  No wave reads another wave's tree:
 * there is no work word, no atomic and no waiting.
 */
#ifndef SUBPROC_AMD_OTHELLO_MCTS_H
#define SUBPROC_AMD_OTHELLO_MCTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTHU_MAX_ITERATIONS 65536
#define OTHU_MAX_NODES (1 << 20)
#define OTHU_MAX_BLOCKS 4096 /* the grid never exceeds this many one-wave blocks (slabs of scratch) */
#define OTHU_NODE_BYTES 32   /* P, O; n, s; d, children */
#define OTHU_PATH_ENTRIES 132 /* a path is at most 2 x empties + 2 nodes long */
#define OTHU_LDS_BYTES 6672  /* ray table 4096 + k-th bit table 2048 + path 132 x 4 */
#define OTHU_SEARCHED 1
#define OTHU_INVALID 2
#define OTHU_NO_MOVE 255

/* Search the n positions boards[i] / turn[i].
 *   iterations 1..OTHU_MAX_ITERATIONS, max_nodes 1..OTHU_MAX_NODES, else
 *              OTH_EINVAL
 *   log_table  float32[iterations + 1], used as given: entry k stands for
 *              ln(max(k, 1)).  The library never computes a logarithm, so the
 *              device, a host build and a checker that share the table agree
 *              bit for bit.  NULL: OTH_EINVAL.
 *   scratch    scratch_bytes >= othu_mcts_scratch_bytes(n, max_nodes) of device
 *              memory, 16-byte aligned, contents irrelevant before and after,
 *              not shared with a launch that may overlap.
 * n == 0: OTH_OK, nothing launched.  n < 0: OTH_EINVAL.
 * OTH_MCTS_BLOCKS in the environment (read per launch) caps the grid as
 * OTH_SEARCH_BLOCKS caps othm_search's; results do not depend on it. */
int othu_mcts(const uint64_t* boards, const uint8_t* turn, int iterations, float explore, const float* log_table,
              uint64_t seed, uint64_t game_id0, int max_nodes, uint32_t* visits, uint32_t* wins, int32_t* diffs,
              uint32_t* root_wins, int32_t* root_diffs, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
              void* scratch, int64_t scratch_bytes, int64_t n, void* stream);

/* bytes of scratch for n positions and trees of max_nodes nodes:
 * min(n, OTHU_MAX_BLOCKS) slabs of OTHU_NODE_BYTES * max_nodes (at least 16;
 * OTH_EINVAL for n < 0 or max_nodes outside 1..OTHU_MAX_NODES) */
int64_t othu_mcts_scratch_bytes(int64_t n, int max_nodes);

/* blocks a call on n positions launches (no launch; cf. othm_search_grid): the
 * device's resident blocks under OTH_MCTS_BLOCKS and OTHU_MAX_BLOCKS, at most n */
int othu_mcts_grid(int64_t n);

#ifdef __cplusplus
}
#endif
#endif
