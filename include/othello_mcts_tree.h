/*
 * othello_mcts_tree.h — C-ABI of the Monte Carlo search trees that persist, of
 * libsubproc_amd_hip.so (subproc_amd/csrc/mcts_tree.hip, gfx950): the trees of
 * othello_mcts.h kept in the caller's device memory, so that a search can be
 * resumed and a tree re-rooted on the move that was played.  DESIGN.md §29.
 *
 * Conventions as in othello_mcts.h.  The functions of this header are prefixed
 * othr_ (no other header's set).
 *
 * THE RULE is othello_mcts.h's: its node, its steps 1 to 4 of an iteration and
 * its rows, referred to below by those names.  This header adds where a tree
 * lives and four operations on it.  The outputs are a function of the inputs
 * and of the trees' contents only.
 *
 * A tree is the node array of othello_mcts.h in slab i of `slabs`, and record i
 * of `records`.  Both belong to the caller, persist between calls, and are
 * written by these calls only; all calls on a set of trees take the same
 * max_nodes M and run in stream order.
 *
 *   slab i     at byte i * 2 * M * OTHU_NODE_BYTES: two halves of M nodes.  The
 *              first half is the tree, as three arrays:
 *                  uint64 pos[M][2]    the mover's discs P, the other side's O
 *                  uint32 ns[M][2]     visits n, half-points s
 *                  uint32 dl[M][2]     disc sum d (int32), children
 *              with children = first | cnt << 20, 0 where the node is not
 *              expanded.  Only the nodes below `nodes` mean anything.  The
 *              second half is othr_advance's room: contents irrelevant.
 *   record i   OTHR_RECORD_BYTES at byte i * OTHR_RECORD_BYTES:
 *                  uint64 id_base      the id of the tree's first playout
 *                  uint64 played       iterations ever run on this tree; only
 *                                      othr_init resets it
 *                  uint32 nodes        the node count
 *                  uint32 turn         the root mover's colour, 1 Black 2 White
 *                  uint32 status       OTHR_READY or OTHR_INVALID: the last
 *                                      status of a call that changed the tree
 *                  uint32 max_nodes    the M the tree was made with
 *              A record whose status is not OTHR_READY, or whose max_nodes is
 *              not the call's, is an INVALID tree: no call but othr_init reads
 *              or writes its slab, every row is 0 and best_move 255.  (So
 *              zeroed records are safe to pass; memory that was never written
 *              is not.)
 *
 * INIT(boards, turn, id_base).  The tree becomes the root alone, n = s = d = 0,
 * nodes = 1, played = 0, status READY.  Black & white overlapping: INVALID,
 * nodes = 0, and it stays INVALID through every later call until the next init.
 *
 * SEARCH(iterations).  With n_root the root's visits, the tree runs
 *     ran = min(iterations_i, OTHU_MAX_ITERATIONS - n_root)
 * more iterations of steps 1 to 4, so that 128 n stays exact in float32 for
 * every node; with ran == 0 the tree and its record are untouched.  Lane j of
 * an iteration plays the game of global id id_base + played * 64 + j (modulo
 * 2^64) of `seed`, then played += 1.  Step 2's "the root" is node 0 of the tree
 * as it stands.  log_table has OTHU_MAX_ITERATIONS + 1 entries and is indexed
 * by n_v as it is.  The outputs are othu_mcts's eight (root_wins stays
 * 128 n_root - s_root: the root mover's count, after a re-root too), `ran`, and
 * the root position as root_boards [black, white] and root_turn.
 *
 * ROWS.  The same outputs, ran = 0, no iteration run.
 *
 * ADVANCE(move, keep).  move 255 leaves the tree as it is (status READY).
 * Otherwise the move must be a legal square of the root mover, or OTH_PASS
 * where the root mover has no move and the other side has one; anything else
 * (an occupied or non-flipping square, a pass while a move exists, any move at
 * a finished game, a code above 64) answers OTHR_BADMOVE and leaves slab and
 * record unchanged, byte for byte.  With keep != 0 and an expanded root the
 * child the move reaches becomes node 0 with its n, s, d and its whole
 * subtree; everything else is dropped and `nodes` becomes the subtree's size,
 * so the tree has room to grow again.  With keep == 0, or a root that is not
 * expanded, the new tree is the child position alone, n = s = d = 0, nodes = 1.
 * `turn` flips, across a pass too.  id_base and played stay.
 *
 * The renumbering.  The kept nodes are renumbered breadth first below the new
 * root, each node's children contiguous and in their order.  Nothing observable
 * depends on which such numbering is used: selection goes through a node's
 * children by sibling order (the first unvisited one, ties of the score to the
 * lowest sibling), expansion appends at `nodes` and depends on the count alone,
 * the rows are read through the root's children in square order, and no output
 * is a node index.  A test that compares trees therefore compares them in a
 * canonical order (breadth first), not index by index.
 *
 * Two consequences.
 *   Resume.  With the same seed, c and M, init with id_base[i] = game_id0 +
 *   i * T * 64 followed by searches of T1, T2, ... that sum to T gives, on
 *   every field, othu_mcts's answer for T (given the same logarithms).
 *   Fresh tree.  After advance(keep = 0), a search of T gives the row that
 *   othu_mcts gives on the child position alone with game_id0 = id_base +
 *   played * 64.
 *
 * How.  Search and advance run one wave per tree, trees assigned to the blocks
 * statically, grid-stride, the grid capped by OTH_MCTS_BLOCKS and the device's
 * resident blocks; tree i is in slab i whatever the grid.  The advance copies
 * the kept subtree breadth first into the slab's second half, the copy being
 * its own queue, and back: time linear in the node count.  No wave reads
 * another wave's tree: nothing atomic, nothing at agent scope, no waiting.
 */
#ifndef SUBPROC_AMD_OTHELLO_MCTS_TREE_H
#define SUBPROC_AMD_OTHELLO_MCTS_TREE_H

#include <stdint.h>

#include "othello_mcts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OTHR_RECORD_BYTES 32
#define OTHR_LDS_BYTES 6672 /* the search kernel's: OTHU_LDS_BYTES; rows and advance use none */
#define OTHR_READY 1        /* OTHU_SEARCHED */
#define OTHR_INVALID 2      /* OTHU_INVALID */
#define OTHR_BADMOVE 8
#define OTHR_KEEP 255       /* othr_advance's move that leaves the tree as it is */

/* bytes of `slabs` for n trees of max_nodes nodes: n * 2 * max_nodes *
 * OTHU_NODE_BYTES (at least 16; OTH_EINVAL for n < 0 or max_nodes outside
 * 1..OTHU_MAX_NODES) */
int64_t othr_trees_slab_bytes(int64_t n, int max_nodes);

/* bytes of `records` for n trees: n * OTHR_RECORD_BYTES (at least 16;
 * OTH_EINVAL for n < 0) */
int64_t othr_trees_record_bytes(int64_t n);

/* blocks a search or an advance of n trees launches (no launch; cf.
 * othu_mcts_grid): the device's resident blocks under OTH_MCTS_BLOCKS and
 * OTHU_MAX_BLOCKS, at most n */
int othr_trees_grid(int64_t n);

/* Every call below: slabs (16-byte aligned) and records (8-byte aligned) with
 * slab_bytes >= othr_trees_slab_bytes(n, max_nodes) and record_bytes >=
 * othr_trees_record_bytes(n), else OTH_EINVAL; max_nodes outside
 * 1..OTHU_MAX_NODES: OTH_EINVAL; n == 0: OTH_OK, nothing launched; n < 0:
 * OTH_EINVAL. */

/* INIT.  turn as in othu_mcts (NULL: Black).  id_base[i] if id_base is given,
 * else game_id0 + i * stride (modulo 2^64). */
int othr_init(const uint64_t* boards, const uint8_t* turn, const uint64_t* id_base, uint64_t game_id0, uint64_t stride,
              int max_nodes, void* slabs, int64_t slab_bytes, void* records, int64_t record_bytes, int64_t n,
              void* stream);

/* SEARCH.  iterations_per_tree[i] if given, else `iterations` for every tree
 * (0..OTHU_MAX_ITERATIONS, else OTH_EINVAL).  log_table: float32
 * [OTHU_MAX_ITERATIONS + 1], as othu_mcts uses its table; NULL: OTH_EINVAL.
 * Every output may be NULL.  status: OTHR_READY or OTHR_INVALID. */
int othr_search(int iterations, const uint32_t* iterations_per_tree, float explore, const float* log_table,
                uint64_t seed, int max_nodes, uint32_t* visits, uint32_t* wins, int32_t* diffs, uint32_t* root_wins,
                int32_t* root_diffs, uint8_t* best_move, uint8_t* status, uint32_t* nodes, uint32_t* ran,
                uint64_t* root_boards, uint8_t* root_turn, void* slabs, int64_t slab_bytes, void* records,
                int64_t record_bytes, int64_t n, void* stream);

/* ROWS: othr_search's outputs with no iteration run (ran = 0 everywhere). */
int othr_rows(int max_nodes, uint32_t* visits, uint32_t* wins, int32_t* diffs, uint32_t* root_wins, int32_t* root_diffs,
              uint8_t* best_move, uint8_t* status, uint32_t* nodes, uint32_t* ran, uint64_t* root_boards,
              uint8_t* root_turn, void* slabs, int64_t slab_bytes, void* records, int64_t record_bytes, int64_t n,
              void* stream);

/* ADVANCE.  move[i] (NULL: OTH_EINVAL); status[i] (may be NULL): OTHR_READY,
 * OTHR_INVALID or OTHR_BADMOVE. */
int othr_advance(const uint8_t* move, int keep, int max_nodes, uint8_t* status, void* slabs, int64_t slab_bytes,
                 void* records, int64_t record_bytes, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
