/*
 * othello_solve.h — C-ABI of the exact endgame solver of libsubproc_amd_hip.so
 * (subproc_amd/csrc/solve.hip, gfx950).  Conventions as in othello.h: boards
 * are 2 x uint64 [black, white] per position, every pointer is DEVICE memory
 * owned by the caller, calls are asynchronous on `stream`, allocate nothing,
 * never synchronise, and return OTH_OK, OTH_EINVAL or -(hipError_t).
 *
 * The functions of this header are prefixed oths_ (the oth_ set of othello.h is
 * shared with the host library oracle/libothello_cpu.so, which has no solver).
 *
 * Value.  For position i with mover m (White if turn[i] == 2, else Black:
 * oth_rollout's rule for start_turn; turn == NULL: Black everywhere),
 *   V(pos, m) = max over m's legal moves of -V(child, opponent)
 *             = -V(pos, opponent)               if m must pass and the opponent can move
 *             = discs(m) - discs(opponent)       if neither side can move.
 * The last line is the project's result rule (game_runner.py:194-199,
 * oth_result's diff seen by the mover): the plain disc difference, with NO
 * bonus for empty squares.  Edax and most endgame solvers give the empties to
 * the winner, so their scores differ on games that end with empty squares.
 *
 * Best move: the LOWEST square among the maximising moves (the library's tie
 * rule); 64 (OTH_PASS) when the mover must pass and the game goes on;
 * OTHS_NO_MOVE when the game is over.
 *
 * The search is alpha-beta, moves lowest square first, no hash table; one GPU
 * lane per position.  Its cost grows by a factor of about 3 to 4 per empty
 * square.
 */
#ifndef SUBPROC_AMD_OTHELLO_SOLVE_H
#define SUBPROC_AMD_OTHELLO_SOLVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 12: at 11 stored frames of 28 B per lane a one-wave block takes 19.25 KB of
 * LDS and eight blocks share a CU (two waves per SIMD); 13 would cost one of
 * them. */
#define OTHS_MAX_EMPTIES 12
#define OTHS_SKIPPED 0 /* more empties than max_empties: value 0, best_move 255, nodes 0 */
#define OTHS_SOLVED 1
#define OTHS_INVALID 2 /* black & white overlap: value 0, best_move 255, nodes 0 */
#define OTHS_LIMIT 3   /* node_limit reached: value and best_move are 0 / 255 */
/* 4 is OTHE_NOROOM (othello_solve_tree.h) */
#define OTHS_BADWINDOW 5 /* othello_solve_window.h: the position's window is out of range or empty */
#define OTHS_NO_MOVE 255
#define OTHS_DEFAULT_NODE_LIMIT (1u << 28)

/* Solve the n positions boards[i] / turn[i] that have at most max_empties
 * (0..OTHS_MAX_EMPTIES, else OTH_EINVAL) empty squares.
 *   value     int8[n]   V as above, from the mover's side
 *   best_move uint8[n]
 *   status    uint8[n]  OTHS_SKIPPED / SOLVED / INVALID / LIMIT
 *   nodes     uint32[n] moves placed and passes made while searching position
 *             i, saturating at the limit; a function of the position, the
 *             mover and the build only (not of n, the neighbours or the grid).
 *             A diagnostic: nothing may compare it across builds.
 * Each of the four may be NULL.  node_limit bounds every position's search
 * (0 = OTHS_DEFAULT_NODE_LIMIT): a position that would need more ends as
 * OTHS_LIMIT, one that needs exactly node_limit is solved.  It is also what
 * bounds the kernel's run time: pass one sized to the time you can wait.
 * work: one device word, 0 at launch, left at 0 — oth_rollout's contract; a
 * stream's launches may share one word between rollouts and solves.
 * n == 0: OTH_OK, nothing launched.
 * OTH_SOLVE_BLOCKS in the environment (read per launch) caps the grid, from 1
 * to the resident count; results do not depend on it. */
int oths_solve(const uint64_t* boards, const uint8_t* turn, int max_empties, uint32_t node_limit,
               int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
               uint64_t* work, int64_t n, void* stream);

/* blocks a solve of n positions launches (no launch; cf. oth_rollout_grid) */
int oths_solve_grid(int64_t n);

#ifdef __cplusplus
}
#endif
#endif
