/*
 * othello_search.h — C-ABI of the depth-limited search of libsubproc_amd_hip.so
 * (subproc_amd/csrc/search.hip, gfx950).  Conventions as in othello_solve.h:
 * boards are 2 x uint64 [black, white] per position, every pointer is DEVICE
 * memory owned by the caller EXCEPT `weights` (host), calls are asynchronous on
 * `stream`, allocate nothing, never synchronise, and return OTH_OK, OTH_EINVAL
 * or -(hipError_t).
 *
 * The functions of this header are prefixed othm_ (oth_ is othello.h's set,
 * shared with the host library; oths_ is the exact solver's).
 *
 * Value.  Position i is searched `depth` plies deep for its root mover r (White
 * if turn[i] == 2, else Black: the solver's rule; turn == NULL: Black
 * everywhere) with the eval table W (int8 [4][9], oth_eval's).  For side to
 * move s with d plies left, S(pos, s, d) is the first line that applies:
 *   1. neither side can move:  T * (discs(s) - discs(opponent)), T = 2^17
 *      (the project's result rule, no bonus for empty squares; |oth_eval| <=
 *      9 * 128 * 64 = 73,728 < T, so a decided game outranks any eval);
 *   2. d == 0:  +oth_eval(pos, r, W) if s == r, else -oth_eval(pos, r, W): the
 *      leaf is always scored from the ROOT mover's view, the eval the 1-ply
 *      policy OTH_POLICY_EVAL maximises (depth 1 chooses that policy's move);
 *   3. s cannot move, the opponent can:  -S(pos, opponent, d): a pass costs no
 *      depth;
 *   4. otherwise:  max over s's legal moves of -S(child, opponent, d - 1).
 * value[i] = S(pos_i, r, depth).  With depth >= the number of empty squares the
 * whole tree is searched: value = T * oths_solve's value, with its move.
 *
 * Best move: the LOWEST square among the maximising moves; 64 (OTH_PASS) when
 * the root mover must pass and the game goes on; OTHM_NO_MOVE when the game is
 * over at the root.
 *
 * The search is alpha-beta, moves lowest square first, fail-hard, no hash
 * table, no move ordering; one GPU lane per position.
 */
#ifndef SUBPROC_AMD_OTHELLO_SEARCH_H
#define SUBPROC_AMD_OTHELLO_SEARCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 8: a leaf is scored where it is made, so depth D stores D - 1 frames of 36 B
 * per lane; at 7 frames a one-wave block takes 15.9 KB of LDS and eight blocks
 * share a CU. */
#define OTHM_MAX_DEPTH 8
#define OTHM_TERMINAL_SCALE (1 << 17) /* T */
#define OTHM_SEARCHED 1
#define OTHM_INVALID 2 /* black & white overlap: value 0, best_move 255, nodes 0 */
#define OTHM_LIMIT 3   /* node_limit reached: value and best_move are 0 / 255 */
#define OTHM_NO_MOVE 255
#define OTHM_DEFAULT_NODE_LIMIT (1u << 28)

/* Search the n positions boards[i] / turn[i] to `depth` plies (1..OTHM_MAX_DEPTH,
 * else OTH_EINVAL).
 *   weights   HOST int8[36], [phase][feature] as oth_eval's; copied into the
 *             launch (NULL: OTH_EINVAL)
 *   value     int32[n]  S as above, from the root mover's side
 *   best_move uint8[n]
 *   status    uint8[n]  OTHM_SEARCHED / INVALID / LIMIT
 *   nodes     uint32[n] moves placed and passes made while searching position
 *             i, saturating at the limit; a function of the position, the
 *             mover, the depth, the table and the build only (not of n, the
 *             neighbours or the grid).  A diagnostic: nothing may compare it
 *             across builds.
 * Each of the four may be NULL.  node_limit bounds every position's search
 * (0 = OTHM_DEFAULT_NODE_LIMIT): a position that would need more ends as
 * OTHM_LIMIT, one that needs exactly node_limit is searched.  It is also what
 * bounds the kernel's run time: pass one sized to the time you can wait.
 * work: one device word, 0 at launch, left at 0 — oth_rollout's contract; a
 * stream's launches may share one word between rollouts, solves and searches.
 * n == 0: OTH_OK, nothing launched.
 * OTH_SEARCH_BLOCKS in the environment (read per launch) caps the grid, from 1
 * to the resident count; results do not depend on it. */
int othm_search(const uint64_t* boards, const uint8_t* turn, int depth, const int8_t* weights,
                uint32_t node_limit, int32_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
                uint64_t* work, int64_t n, void* stream);

/* blocks a search of n positions launches (no launch; cf. oths_solve_grid) */
int othm_search_grid(int64_t n);

#ifdef __cplusplus
}
#endif
#endif
