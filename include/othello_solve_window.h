/*
 * othello_solve_window.h — C-ABI of the exact endgame solvers WITH A ROOT
 * WINDOW (subproc_amd/csrc/solve.hip, solve_tree.hip, gfx950): oths_solve
 * (othello_solve.h), othe_solve (othello_solve_tree.h) and othh_solve_hashed
 * (othello_solve_hash.h) asked a cheaper question than the exact disc
 * difference.  DESIGN.md §20.
 *
 * Conventions as in those headers.  The functions of this header are prefixed
 * othw_ (a set of its own, as each of the library's headers has).
 *
 * The window.  Position i has a window (alpha[i], beta[i]) with
 * OTHW_ALPHA_MIN <= alpha < beta <= OTHW_BETA_MAX, seen from the side of the
 * root's mover.  alpha and beta are int8 DEVICE arrays of n; either may be
 * NULL, which is OTHW_ALPHA_MIN (resp. OTHW_BETA_MAX) everywhere.  With V the
 * exact value of othello_solve.h (the same three rules, no bonus for empties):
 *   value      clamp(V, alpha, beta), exactly (the search is fail-hard).
 *   best_move  for a root whose mover has a move:
 *                alpha < V < beta   the LOWEST square among the maximisers;
 *                V >= beta          the LOWEST square among the moves whose own
 *                                   value is >= beta;
 *                V <= alpha         OTHS_NO_MOVE: no move is proved;
 *              64 (OTH_PASS) for a forced pass at the root and OTHS_NO_MOVE
 *              for a finished game, whatever the window.
 *   status     OTHS_SKIPPED, OTHS_INVALID, OTHS_LIMIT and OTHE_NOROOM as in the
 *              headers above, and classified first.  A position that would
 *              otherwise be searched and whose window is out of range or has
 *              alpha >= beta ends as OTHS_BADWINDOW (othello_solve.h) with
 *              value 0, best_move OTHS_NO_MOVE and nodes 0.
 * They are functions of the position, the mover and the window only: in the
 * split solver they do not depend on timing, the order of the tasks, the grid,
 * the table or `order` (node_limit's own exception in othello_solve_hash.h
 * holds).
 *
 * The full window (-65, 65), or both pointers NULL, gives bit for bit what
 * the call without a window gives, othw_solve's `nodes` included.
 *
 * Win / draw / loss is the window (-1, +1): the value is the sign of V, the
 * move the lowest winning move on a win, the lowest drawing move on a draw and
 * OTHS_NO_MOVE on a loss.
 */
#ifndef SUBPROC_AMD_OTHELLO_SOLVE_WINDOW_H
#define SUBPROC_AMD_OTHELLO_SOLVE_WINDOW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTHW_ALPHA_MIN (-65)
#define OTHW_BETA_MAX 65

/* oths_solve (othello_solve.h: every other argument, check and result as
 * there) with each position's window.  One GPU lane per position, at most
 * OTHS_MAX_EMPTIES empties.  A narrower window never costs a position more
 * nodes than the full one.  work: one device word, 0 at launch, left at 0.
 * n == 0: OTH_OK, nothing launched. */
int othw_solve(const uint64_t* boards, const uint8_t* turn, const int8_t* alpha, const int8_t* beta, int max_empties,
               uint32_t node_limit, int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
               uint64_t* work, int64_t n, void* stream);

/* othe_solve (othello_solve_tree.h) with each position's window and,
 * optionally, othh_solve_hashed's table (othello_solve_hash.h).  table == NULL
 * with hash_bits == 0: no table (hash_min_empties and table_bytes are not
 * looked at).  Otherwise the table arguments are checked as othh_solve_hashed
 * checks them (OTH_EINVAL, before anything else, also for n == 0).  A table
 * filled by windowed calls is valid input to calls without a window and the
 * other way round: an entry is a bound on the exact value whatever window
 * proved it.
 * The root is not cut off when it reaches beta: every root move is resolved
 * (the later ones in the window (beta - 1, beta)), which is what makes the
 * move above knowable. */
int othw_solve_split(const uint64_t* boards, const uint8_t* turn, int max_empties, int task_empties, int order,
                     uint32_t node_limit, int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
                     void* scratch, int64_t scratch_bytes, int32_t nodes_per_position, uint64_t* work, int64_t n,
                     const int8_t* alpha, const int8_t* beta, int hash_bits, int hash_min_empties, void* table,
                     int64_t table_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
