/*
 * othello_perft.h — C-ABI of perft of libsubproc_amd_hip.so
 * (subproc_amd/csrc/perft.hip, gfx950): the number of move paths of a given
 * length from each position of a batch.  DESIGN.md §27.
 *
 * Conventions as in othello_solve.h: boards are 2 x uint64 [black, white] per
 * position, every pointer is DEVICE memory owned by the caller, calls are
 * asynchronous on `stream`, allocate nothing, never synchronise, and return
 * OTH_OK, OTH_EINVAL or -(hipError_t).
 *
 * The functions of this header are prefixed othc_ (oth_, oths_, othm_, othp_,
 * otht_, otho_, othe_, othh_, othw_, otha_, othb_, othl_ and othx_ are the
 * other headers' sets).
 *
 * The rule.  For position pos, side to move s (White if turn[i] == 2, else
 * Black; turn == NULL: Black everywhere) and d plies left:
 *
 *   N(pos, s, 0) = 1
 *   N(pos, s, d) = sum over s's legal moves m of N(pos after m, opponent, d - 1)
 *                                                      if s has a move
 *                = N(pos, opponent, d - 1)             if s must pass
 *                = 1                                   if neither side can move
 *
 * A PASS IS A PLY, and a finished game is one path however many plies are
 * left.  This is the published convention of Othello perft (from the opening,
 * Black to move: 4, 12, 56, 244, 1396, 8200, 55092, 390216, 3005288, 24571284,
 * 212258800, 1939886636 at depths 1..12).  It is NOT the rule of the searches
 * of this library (othello_search.h rule 3, othello_solve.h), where a pass
 * costs no depth: depth 9 from the opening is the first where the two differ.
 *
 * Outputs, per position i:
 *   leaves[i]           N(pos_i, mover_i, depth_i)
 *   divide[i * 64 + s]  N(pos_i after s, opponent, depth_i - 1) for every legal
 *                       root move s, 0 elsewhere; the row is all 0 when the
 *                       root mover must pass, when the game is over and when
 *                       depth_i == 0.  Where the row is not all 0 it sums to
 *                       leaves[i].
 *   status[i]           OTHC_COUNTED;
 *                       OTHC_INVALID: black & white overlap, leaves 0, row 0;
 *                       OTHC_LIMIT: one of the position's tasks (below) ran
 *                       into node_limit, leaves 0, row 0;
 *                       OTHC_BADDEPTH: depths[i] > OTHC_MAX_DEPTH, leaves 0,
 *                       row 0.
 *   nodes[i]            the positions whose moves the counting kernel generated
 *                       for position i (the expansion's own are not counted).
 *                       A diagnostic: it depends on split and on the room.
 * leaves, divide and status are a function of the position, the mover and the
 * depth ONLY: not of split, max_tasks, the grid, the neighbours or timing
 * (integer sums commute), as long as no task meets node_limit.
 *
 * How.  Every valid position starts as one task: (mover's discs, other
 * side's discs, a word holding the position's index, its root square, the
 * plies left and an "over" flag), 24 B.  `split` expand kernels then replace,
 * level by level, every task of the list by its children (one ply fewer), by
 * one swapped child for a pass, by itself flagged "over" when neither side can
 * move, or by itself when it has no ply left or is over already; the first
 * level tags every task with its root move (OTH_PASS for a root pass: no
 * column).  The lists ping-pong between two halves of `scratch`.  A level
 * whose tasks do not fit the list is VOID: it raises a flag, later levels
 * return at once and the level before it stays in force — nothing is read on
 * the host, the call may be captured in a graph and never fails for lack of
 * room.  The count kernel — search.hip's persistent one-wave loop, lanes
 * claiming tasks through the work word — walks each task's tree with frames
 * in LDS and adds its count to leaves[i] (and to the task's column of the row)
 * with one 64-bit atomic; the last ply is counted in bulk (popcount of the move
 * mask, no flips).  A finish kernel writes status and clears the counts of a
 * position whose task met the limit.
 *
 * No sum wraps: a list holds at most OTHC_MAX_TASKS = 2^24 tasks, a task
 * generates at most node_limit <= 2^32 positions, and a generated position
 * adds at most 64 (its moves; no reachable position has more than 33), so
 * leaves <= 64 * 2^24 * 2^32 = 2^62 < 2^63: the counts also fit int64.
 */
#ifndef SUBPROC_AMD_OTHELLO_PERFT_H
#define SUBPROC_AMD_OTHELLO_PERFT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 14: the frame on top is in registers and a node with one ply left is never
 * pushed, so 13 frames of 24 B per lane: a one-wave block takes
 * OTHC_COUNT_LDS_BYTES of LDS and eight blocks share a CU. */
#define OTHC_MAX_DEPTH 14
#define OTHC_COUNT_LDS_BYTES 19968 /* 13 frames x 6 words x 64 lanes x 4 B */
#define OTHC_MAX_SPLIT 8
#define OTHC_MAX_TASKS (1 << 24)
#define OTHC_ROOT_SLOTS 64 /* room per position that a divide row asks for */
#define OTHC_COUNTED 1
#define OTHC_INVALID 2
#define OTHC_LIMIT 3
#define OTHC_BADDEPTH 7 /* (4, 5 and 6 are OTHE_NOROOM, OTHS_BADWINDOW and OTHL_BADDEPTH) */
#define OTHC_DEFAULT_NODE_LIMIT (1u << 28)

/* Count the move paths of the n positions boards[i] / turn[i].
 *   depth      0..OTHC_MAX_DEPTH, else OTH_EINVAL; used where depths == NULL
 *   depths     uint8[n] or NULL: a depth per position (one above
 *              OTHC_MAX_DEPTH ends that position as OTHC_BADDEPTH)
 *   split      0..OTHC_MAX_SPLIT expand levels, else OTH_EINVAL.  0: a lane
 *              walks a whole position.  A divide row needs the root moves as
 *              tasks, so with divide != NULL at least one level is made.
 *   node_limit bounds the positions EACH TASK may generate
 *              (0 = OTHC_DEFAULT_NODE_LIMIT); it is also what bounds the run
 *              time of a lane.
 *   leaves uint64[n]; divide uint64[n][64]; status uint8[n]; nodes uint64[n];
 *              each may be NULL.
 *   scratch    scratch_bytes >= othc_perft_scratch_bytes(n, max_tasks) of
 *              device memory, 16-byte aligned, contents irrelevant before and
 *              after, not shared with a launch that may overlap.  The lists
 *              hold as many tasks as the bytes given allow, at most
 *              OTHC_MAX_TASKS.  With divide != NULL the lists must hold
 *              OTHC_ROOT_SLOTS * n tasks, so that the first level always fits
 *              and the row does not depend on the room: else OTH_EINVAL.
 *   work       one device word, 0 at launch, left at 0 (oth_rollout's
 *              contract); may be shared with the other calls of a stream.
 * n == 0: OTH_OK, nothing launched.  n > OTHC_MAX_TASKS: OTH_EINVAL.
 * OTH_PERFT_BLOCKS in the environment (read per launch) caps the count
 * kernel's and the expand kernels' grids as OTH_SEARCH_BLOCKS caps
 * othm_search's; results do not depend on it. */
int othc_perft(const uint64_t* boards, const uint8_t* turn, int depth, const uint8_t* depths, int split,
               uint32_t node_limit, uint64_t* leaves, uint64_t* divide, uint8_t* status, uint64_t* nodes,
               void* scratch, int64_t scratch_bytes, uint64_t* work, int64_t n, void* stream);

/* bytes of scratch for n positions and lists of max(max_tasks, n, 1) tasks
 * (OTH_EINVAL for n < 0, max_tasks < 0, or more than OTHC_MAX_TASKS of either) */
int64_t othc_perft_scratch_bytes(int64_t n, int64_t max_tasks);

/* blocks the count kernel of a call on n positions launches at most (no
 * launch; cf. othm_search_grid): the device's resident blocks under
 * OTH_PERFT_BLOCKS */
int othc_perft_grid(int64_t n);

#ifdef __cplusplus
}
#endif
#endif
