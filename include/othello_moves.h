/*
 * othello_moves.h — C-ABI of the analysis calls of libsubproc_amd_hip.so
 * (subproc_amd/csrc/moves.hip, gfx950): the value of EVERY root move, from the
 * exact solvers and from the depth-limited search.  DESIGN.md §21.
 *
 * Conventions as in othello_solve.h: boards are 2 x uint64 [black, white] per
 * position, every pointer is DEVICE memory owned by the caller EXCEPT the
 * search's `weights` (host), calls are asynchronous on `stream`, allocate
 * nothing, never synchronise, and return OTH_OK, OTH_EINVAL or -(hipError_t).
 *
 * The functions of this header are prefixed otha_ (oth_, oths_, othm_, othp_,
 * otht_, otho_, othe_, othh_ and othw_ are the other headers' sets).
 *
 * Semantics, the same for all three calls.  Position i has root mover r (White
 * if turn[i] == 2, else Black; turn == NULL: Black everywhere).
 *
 * move_value[i * 64 + s], for every square s:
 *   - s is a legal move of r:
 *       exact calls  -V(child_s, opponent), V as in othello_solve.h;
 *       search       -S(child_s, opponent, depth - 1) WITH ROOT MOVER r, by the
 *                    four rules of othello_search.h: every leaf below the move
 *                    is scored from r's side, a game that is over at the child
 *                    scores T times the disc difference, and with depth == 1
 *                    the child is a leaf scored where it is made: the value is
 *                    +oth_eval(child, r).  (othm_search on the child would
 *                    score the leaves from the child's mover's side, and the
 *                    eval is not antisymmetric: it gives other numbers.)
 *   - s is not a legal move: OTHA_NOT_A_MOVE (int8) / OTHA_NOT_A_MOVE32 (int32);
 *   - the move could not be resolved (its subtree hit node_limit, or in the
 *     split call did not fit its slab): OTHA_UNKNOWN / OTHA_UNKNOWN32.
 *
 * value[i], best_move[i]: exactly what oths_solve / othe_solve / othm_search
 * give for the position: the maximum of the row and the LOWEST maximising
 * square.
 *   - forced pass at the root: the row is all OTHA_NOT_A_MOVE, best_move is 64
 *     (OTH_PASS) and value is the value of the passed position.  ONE task
 *     computes it: the same board with the opponent to move.  In the search the
 *     pass costs no depth;
 *   - finished game: the disc difference from r's side (times T in the
 *     search), move 255, the row all OTHA_NOT_A_MOVE;
 *   - any move unknown: 0 and 255, as the existing calls answer at a limit.
 *
 * status[i]: OTHS_SKIPPED (exact calls: more than max_empties empties) and
 * OTHS_INVALID / OTHM_INVALID (black & white overlap) are classified first, as
 * in the existing calls; their rows are all OTHA_NOT_A_MOVE, value 0, move 255,
 * nodes 0.  Otherwise the LARGEST status among the position's tasks:
 * OTHS_SOLVED = OTHM_SEARCHED = 1 < OTHS_LIMIT = OTHM_LIMIT = 3 < OTHE_NOROOM =
 * 4 (a finished game has no task and is 1).
 *
 * nodes[i]: the number of root tasks (one per legal move, or one for the pass)
 * plus the tasks' own counts, summed in 64 bits and saturated to 32.  In the
 * one-lane calls (otha_solve_moves, otha_search_moves) a function of the
 * position, the mover, max_empties or the depth and table, and the build only;
 * in the split call it depends on timing as othe_solve's does.  A diagnostic.
 *
 * node_limit (0 = the existing calls' default, 2^28) bounds EACH ROOT MOVE's
 * subtree, not the position (in the split call each task of each move, as in
 * othe_solve).
 *
 * move_value, value, best_move, status and nodes may each be NULL.
 * work: one device word, 0 at launch, left at 0 (oth_rollout's contract); may
 * be shared with rollouts, solves and searches on the same stream.
 * n == 0: OTH_OK, nothing launched.
 *
 * How.  Three steps on the stream: an expand kernel classifies each position
 * and writes one task per root move (the board after the move, the opponent to
 * move) into `scratch`; the tasks are solved or searched; a finish kernel
 * scatters minus the tasks' values into the rows and reduces value, move,
 * status and nodes per position.  scratch: scratch_bytes >= the call's
 * ..._scratch_bytes() of device memory, 16-byte aligned, contents irrelevant
 * before and after; not shared with a launch that may overlap.
 *
 * Limits: no root window and no `order` for the one-lane calls, no split and
 * no order for the search.
 */
#ifndef SUBPROC_AMD_OTHELLO_MOVES_H
#define SUBPROC_AMD_OTHELLO_MOVES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTHA_NOT_A_MOVE (-128)            /* int8 rows of the exact calls */
#define OTHA_UNKNOWN (-127)
#define OTHA_NOT_A_MOVE32 (-2147483647 - 1) /* int32 rows of the search: INT32_MIN */
#define OTHA_UNKNOWN32 (-2147483647)        /* INT32_MIN + 1 */
#define OTHA_SEARCH_SLOTS 64              /* task slots otha_search_moves_scratch_bytes counts per position */

/* The exact value of every root move by oths_solve's one-lane kernel.
 * 0 <= max_empties <= OTHS_MAX_EMPTIES, else OTH_EINVAL.
 *   move_value int8[n][64]; value int8[n]; best_move uint8[n]; status uint8[n];
 *   nodes uint32[n]
 * The tasks are solved by oths_solve's launch, called internally on a fixed
 * max(max_empties, 1) task slots per position (a solved position has no more
 * moves than empties); unused slots hold the empty board, which that kernel
 * skips at once.  Nothing is counted on the host, so the call may be captured
 * in a graph.  OTH_SOLVE_BLOCKS caps the grid as it does oths_solve's. */
int otha_solve_moves(const uint64_t* boards, const uint8_t* turn, int max_empties, uint32_t node_limit,
                     int8_t* move_value, int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
                     void* scratch, int64_t scratch_bytes, uint64_t* work, int64_t n, void* stream);

/* bytes of scratch otha_solve_moves needs (OTH_EINVAL for n < 0, max_empties
 * out of range or a size beyond 2^55 tasks) */
int64_t otha_solve_moves_scratch_bytes(int64_t n, int max_empties);

/* The same by the split solver: the tasks go through othe_solve, or through
 * othh_solve_hashed when `table` is not NULL (table NULL: hash_bits,
 * hash_min_empties and table_bytes are not read).  0 <= max_empties <=
 * OTHE_MAX_EMPTIES; task_empties, order, nodes_per_position, hash_bits,
 * hash_min_empties, table, table_bytes: othe_solve's and othh_solve_hashed's
 * ranges and checks, else OTH_EINVAL.  EVERY TASK SLOT COSTS A SLAB:
 * otha_solve_moves_split_scratch_bytes grows with n * max(max_empties, 1) *
 * nodes_per_position, so batches want a smaller nodes_per_position than one
 * position does.  A move whose tree does not fit its slab is OTHA_UNKNOWN and
 * the position ends as OTHE_NOROOM. */
int otha_solve_moves_split(const uint64_t* boards, const uint8_t* turn, int max_empties, int task_empties, int order,
                           uint32_t node_limit, int32_t nodes_per_position, int hash_bits, int hash_min_empties,
                           void* table, int64_t table_bytes, int8_t* move_value, int8_t* value, uint8_t* best_move,
                           uint8_t* status, uint32_t* nodes, void* scratch, int64_t scratch_bytes, uint64_t* work,
                           int64_t n, void* stream);

int64_t otha_solve_moves_split_scratch_bytes(int64_t n, int max_empties, int32_t nodes_per_position);

/* The depth-limited value of every root move.  1 <= depth <= OTHM_MAX_DEPTH,
 * weights HOST int8[36] (NULL: OTH_EINVAL), else as othm_search.
 *   move_value int32[n][64]; value int32[n]; best_move uint8[n];
 *   status uint8[n] (OTHM_SEARCHED / INVALID / LIMIT); nodes uint32[n]
 * The expand kernel packs the tasks of all positions into one list (a device
 * counter in scratch, cleared by a memset node on the stream), and
 * search_moves_kernel, search.hip's persistent one-wave loop over tasks,
 * claims them from it.  A depth-1 task is scored when it is claimed.  The
 * scratch is sized for OTHA_SEARCH_SLOTS tasks per position and touched only as
 * far as the moves go.  OTH_SEARCH_BLOCKS caps the grid as it does othm_search's. */
int otha_search_moves(const uint64_t* boards, const uint8_t* turn, int depth, const int8_t* weights,
                      uint32_t node_limit, int32_t* move_value, int32_t* value, uint8_t* best_move, uint8_t* status,
                      uint32_t* nodes, void* scratch, int64_t scratch_bytes, uint64_t* work, int64_t n, void* stream);

int64_t otha_search_moves_scratch_bytes(int64_t n);

#ifdef __cplusplus
}
#endif
#endif
