/*
 * othello_solve_hash.h — C-ABI of the split endgame solver WITH A TRANSPOSITION
 * TABLE (subproc_amd/csrc/solve_tree.hip, solve_hash_core.hpp, gfx950):
 * othello_solve_tree.h's othe_solve with a table of solved positions in device
 * memory, shared by every task of every position of a call and kept by the
 * caller between calls.  DESIGN.md §19.
 *
 * Conventions as in othello_solve_tree.h.  The functions of this header are
 * prefixed othh_ (a set of its own beside oth_, oths_, othm_, othp_, otht_,
 * otho_ and othe_, as each of the library's headers has).
 *
 * Values, moves and statuses are othe_solve's, which are oths_solve's: the
 * exact value, the LOWEST square among the maximisers, 64 for a forced pass,
 * OTHS_NO_MOVE for a finished game; OTHS_SKIPPED, OTHS_INVALID, OTHE_NOROOM and
 * OTHS_LIMIT as there.  They are functions of the position and of othe_solve's
 * arguments.  They NEVER depend on the table's size or contents, on
 * hash_min_empties, on the neighbours, the grid or timing.  The one exception
 * is othe_solve's own for node_limit, which the table widens: a fuller table
 * makes a task cheaper, so a position with a task within reach of node_limit
 * may end as OTHS_LIMIT with one table and as OTHS_SOLVED (with the right
 * value) with another.  `nodes` stays a diagnostic.
 *
 * The table.  2^hash_bits entries of OTHH_ENTRY_BYTES bytes: both bitboards in
 * full, a lower and an upper bound on the position's exact value, and a
 * sequence word.  An entry is used only when both boards equal the prober's
 * word for word, and never as a mix of two writers' words.  The value of a
 * position played to the end is a fact about the position alone, so:
 *   - ALL ZERO IS EMPTY, and the solver never clears the table;
 *   - a table filled by earlier calls of this library is valid input to any
 *     later call, whatever its order, task_empties, max_empties or batch;
 *   - the table is the caller's device memory, OTHH_ENTRY_BYTES-aligned.
 * Launches that may OVERLAP on one table (two streams) are NOT supported.
 * Calls on one stream, one after the other, are the intended use.
 *
 * hash_min_empties: only search frames with at least this many empty squares
 * probe and store; below it a trip to device memory costs more than the
 * subtree.  It is a SPEED knob and never a result knob.
 * The root of a position and the nodes of its expanded top are never answered
 * from the table.
 */
#ifndef SUBPROC_AMD_OTHELLO_SOLVE_HASH_H
#define SUBPROC_AMD_OTHELLO_SOLVE_HASH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTHH_MIN_BITS 4               /* 16 entries: every store replaces */
#define OTHH_MAX_BITS 26              /* 2 GiB */
#define OTHH_ENTRY_BYTES 32
#define OTHH_MIN_EMPTIES_LO 1         /* hash_min_empties' range */
#define OTHH_MIN_EMPTIES_HI 12
#define OTHH_DEFAULT_MIN_EMPTIES 8    /* DESIGN.md §19 has the sweep */

/* othe_solve (othello_solve_tree.h: every argument, check and result as there)
 * with the table.  OTHH_MIN_BITS <= hash_bits <= OTHH_MAX_BITS and
 * OTHH_MIN_EMPTIES_LO <= hash_min_empties <= OTHH_MIN_EMPTIES_HI; table not
 * NULL, OTHH_ENTRY_BYTES-aligned, table_bytes >= othh_hash_bytes(hash_bits);
 * else OTH_EINVAL (checked before anything else, also for n == 0).
 * Asynchronous on `stream`, allocates nothing, never synchronises.
 * n == 0: OTH_OK, nothing launched. */
int othh_solve_hashed(const uint64_t* boards, const uint8_t* turn, int max_empties, int task_empties, int order,
                      uint32_t node_limit, int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
                      void* scratch, int64_t scratch_bytes, int32_t nodes_per_position, uint64_t* work, int64_t n,
                      int hash_bits, int hash_min_empties, void* table, int64_t table_bytes, void* stream);

/* bytes of a table of 2^hash_bits entries (OTH_EINVAL out of range) */
int64_t othh_hash_bytes(int hash_bits);

#ifdef __cplusplus
}
#endif
#endif
