/*
 * othello_line.h — C-ABI of the principal-variation calls of
 * libsubproc_amd_hip.so (subproc_amd/csrc/line.hip, gfx950): the LINE of best
 * play behind a value, from the exact solver and from the depth-limited
 * search.  DESIGN.md §24.
 *
 * Conventions as in othello_moves.h: boards are 2 x uint64 [black, white] per
 * position, every pointer is DEVICE memory owned by the caller EXCEPT the
 * search's `weights` (host), calls are asynchronous on `stream`, allocate
 * nothing, never synchronise, and return OTH_OK, OTH_EINVAL or -(hipError_t).
 *
 * The functions of this header are prefixed othl_ (oth_, oths_, othm_, othp_,
 * otht_, otho_, othe_, othh_, othw_, otha_ and othb_ are the other headers'
 * sets).
 *
 * THE LINE.  Position i has root mover r (White if turn[i] == 2, else Black;
 * turn == NULL: Black everywhere).  A walk holds (position, side to move t,
 * plies left rem); it starts at (root, r, depth) — for the exact call rem is
 * unbounded — and repeats, the first that applies:
 *   1. neither side can move: stop;
 *   2. search only, rem == 0: stop (the leaf whose score the value is);
 *   3. t cannot move and the opponent can: append 64 (OTH_PASS) and hand the
 *      move over; rem is unchanged (a pass costs no depth, othello_search.h);
 *   4. otherwise append the LOWEST square among t's moves that maximise
 *        exact:   -V(child, opponent), V as in othello_solve.h;
 *        search:  -S(child, opponent, rem - 1) WITH ROOT MOVER r, by the four
 *                 rules of othello_search.h, exactly as othello_moves.h states
 *                 it for the root's moves;
 *      play it and decrement rem.
 * So line[0] is best_move of oths_solve / othm_search (64 for a forced pass; a
 * finished game has an empty line and best_move 255); the value from t's side
 * is +value where t == r and -value otherwise at every node of the line; the
 * end position's static score from r's side is the value (the disc difference;
 * in the search oth_eval(end, r) at a leaf or T times the difference where the
 * game is over); and a search line at a depth of at least the number of empty
 * squares is the exact line.  The line is a function of the position (and the
 * depth and table) alone: `order` does not change it.
 *
 * Outputs per position, each may be NULL:
 *   line        uint8[n][OTHL_LINE_STRIDE], padded with 255.  Passes never come
 *               twice in a row, so a line has at most 2 x 12 entries
 *   length      uint8[n]
 *   value       int8[n] (exact) / int32[n] (search), best_move uint8[n],
 *   status      uint8[n], nodes uint32[n]: as oths_solve / othm_search
 *   end_boards  uint64[n][2] [black, white]: the position where the line ends
 *   end_turn    uint8[n]: the side the walk holds to move there (1 / 2)
 * line and end_boards are written 16 bytes at a time: each must be 16-byte
 * aligned (else OTH_EINVAL).
 *
 * status[i]: OTHS_SKIPPED (exact: more than max_empties empties) and
 * OTHS_INVALID / OTHM_INVALID (black & white overlap) are classified first, as
 * in the existing calls: an empty line, value 0, move 255, nodes 0 (end_boards
 * is the position, end_turn its mover).  OTHS_LIMIT / OTHM_LIMIT when any
 * search of the walk would pass node_limit, which bounds EACH search of the
 * walk (0 = the existing calls' default, 2^28): the answer is then all or
 * nothing, an empty line, 0 and 255.  nodes[i] is the sum over the walk's
 * searches, added in 64 bits and saturated to 32: a function of the position,
 * the parameters and the build.
 *
 * How.  One lane per position, the existing one-lane machines unchanged.  When
 * a lane's search ends with value v and move m the lane plays m and searches
 * the child as a root of its own on the window (-v - 1, -v + 1), until the
 * walk stops.  The root search runs on the full window exactly as oths_solve /
 * othm_search do, and for a fixed move order a search on a window inside the
 * one its parent gave it visits a subset of the nodes: with order == 0 a
 * position the existing call resolves under node_limit is resolved here.
 *
 * work: one device word, 0 at launch, left at 0 (oth_rollout's contract); may
 * be shared with rollouts, solves and searches on the same stream.
 * n == 0: OTH_OK, nothing launched.
 *
 * Limits: no line through the split solver or the split search (more than 12
 * empties, more than depth 8), no root window, no line recorded inside
 * othp_play.
 */
#ifndef SUBPROC_AMD_OTHELLO_LINE_H
#define SUBPROC_AMD_OTHELLO_LINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTHL_LINE_STRIDE 32 /* bytes per position in `line` */
#define OTHL_BADDEPTH 6     /* status: the position's depth entry is above OTHM_MAX_DEPTH */

/* The line of perfect play.  0 <= max_empties <= OTHS_MAX_EMPTIES, else
 * OTH_EINVAL.  OTH_SOLVE_BLOCKS caps the grid as it does oths_solve's. */
int othl_solve_line(const uint64_t* boards, const uint8_t* turn, int max_empties, uint32_t node_limit, uint8_t* line,
                    uint8_t* length, int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
                    uint64_t* end_boards, uint8_t* end_turn, uint64_t* work, int64_t n, void* stream);

/* The line of the depth-limited search.  depth_per_position NULL: every
 * position is searched `depth` (1..OTHM_MAX_DEPTH, else OTH_EINVAL) plies
 * deep.  Otherwise `depth` is not read and position i is searched
 * depth_per_position[i] (device uint8[n]) plies deep; an entry of 0 is not
 * searched (an empty line, value 0, move 255, OTHM_LIMIT: the answer
 * othb_search gives a position whose budget did not fit depth 1, so
 * othb_search's `depth` output can be passed straight in), an entry above
 * OTHM_MAX_DEPTH ends as OTHL_BADDEPTH (empty line, 0, 255, nodes 0).
 * OTHM_INVALID is classified before either.  order: 0 or 1 as
 * otho_search_ordered (the line is the same, nodes are not; with order == 1 a
 * position within reach of node_limit may end differently).  weights HOST
 * int8[36] (NULL: OTH_EINVAL).  OTH_SEARCH_BLOCKS caps the grid. */
int othl_search_line(const uint64_t* boards, const uint8_t* turn, int depth, const uint8_t* depth_per_position,
                     int order, const int8_t* weights, uint32_t node_limit, uint8_t* line, uint8_t* length,
                     int32_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes, uint64_t* end_boards,
                     uint8_t* end_turn, uint64_t* work, int64_t n, void* stream);

/* blocks a launch of n positions uses (tests of the grid cap) */
int othl_solve_line_grid(int64_t n);
int othl_search_line_grid(int64_t n, int order);

#ifdef __cplusplus
}
#endif
#endif
