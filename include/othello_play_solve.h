/*
 * othello_play_solve.h — C-ABI of the search self-play whose last plies are the
 * exact solver's, of libsubproc_amd_hip.so (subproc_amd/csrc/play_solve.hip,
 * gfx950).  Conventions as in othello_play.h: boards are 2 x uint64 [black,
 * white], every pointer is DEVICE memory owned by the caller EXCEPT the two
 * weight tables (host), calls are asynchronous on `stream`, allocate nothing,
 * never synchronise, and return OTH_OK, OTH_EINVAL or -(hipError_t).
 *
 * The functions of this header are prefixed othx_ (othp_ is the games' set,
 * othb_ the budget searches', otho_ the ordered calls', oths_ the solver's).
 *
 * THE RULE.  A game is othello_play.h's game, draw for draw and turn for turn:
 * the colour draw, the random-move budgets, the coin on every turn of a player
 * with budget left (a pass included), game over / pass / coin / single move,
 * and OTHP_MAX_PLIES.  Only rule 4 of its turn changes.  With E = solve_empties
 * (1..OTHS_MAX_EMPTIES, the same for both players):
 *   4. when the position has at most E empty squares, the policy move is
 *      oths_solve's best_move for the position and the mover: the lowest square
 *      among the maximisers of the exact value on the full window.  Above E
 *      empties it is the search's move as in othp_play / otho_play_ordered
 *      (budget_a == budget_b == 0: fixed depth) or as in othb_play (both
 *      budgets >= 1: by budget, the depths being the caps).
 *
 * What follows from it:
 *   - For E <= OTHM_MAX_DEPTH the games are, field for field except nodes,
 *     those of the existing call with exact_empties = E: a search that reaches
 *     the end of the game gives the solver's move (othello_search.h, "Value").
 *   - node_limit (0 = OTHM_DEFAULT_NODE_LIMIT, which is the solver's default
 *     too) bounds every search AND every solve the call runs.  A game whose
 *     search or solve would pass it stops there as OTHM_LIMIT, with the outputs
 *     othp_play gives such a game.
 *   - When the previous ply was the solver's own choice with value v, the next
 *     policy turn's solve runs on the window (-v - 1, -v + 1) instead of the
 *     full one: the move is the same, the tree is smaller.
 *     After a coin move, a single move, a pass, or where a game enters the
 *     zone, the solve runs on the full window.  WHICH solves meet node_limit is
 *     therefore a property of the build; for a given game, arguments and build
 *     it is deterministic.
 *   - nodes[i] stays a diagnostic: the game's search nodes plus its solve nodes.
 *   - order applies to the searches, as today.  The solves run
 *     solve_core.hpp's machine in square order under either setting; the games
 *     do not depend on it.
 *
 * HOW IT RUNS.  Two launches behind the one call.  The first is the existing
 * games' loop; a game whose turn begins with at most E empty squares (its start
 * included) is parked: its state goes into a list in `scratch`, counted by a
 * device counter there that a node of the call itself zeroes.  Games that end
 * above the zone are written as today.  The second launch's lanes take the
 * parked games up, 64 lanes to a block with the solver's stack in LDS, and play
 * each to its end.  One lane plays one game's endgame: the call lasts as long
 * as its hardest game's solves.
 *
 * Not here (limits): an E per player; a win/draw/loss zone above
 * E; more than OTHS_MAX_EMPTIES empties or the split solver inside a game; a
 * transposition table; one game's solve split over lanes.
 */
#ifndef SUBPROC_AMD_OTHELLO_PLAY_SOLVE_H
#define SUBPROC_AMD_OTHELLO_PLAY_SOLVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTHX_COUNTER_BYTES 16 /* the parked list's counter (one uint64) and its padding */
#define OTHX_PARKED_BYTES 48  /* a parked game: boards, RNG, index, nodes, ply / budgets / colours */

/* Play the n games.  Arguments, outputs, statuses and hist are othp_play's
 * (othello_play.h); `order` is otho_play_ordered's (0 or 1), budget_a /
 * budget_b othb_play's.
 *   budget_a / budget_b  0, 0: fixed depth; else both >= 1: by budget, depth_a /
 *                        depth_b are the caps.  One zero, the other not:
 *                        OTH_EINVAL
 *   solve_empties        1..OTHS_MAX_EMPTIES, else OTH_EINVAL
 *   scratch              device memory, 16-byte aligned, of at least
 *                        othx_scratch_bytes(n) bytes (scratch_bytes says how
 *                        many); NULL, misaligned or too small: OTH_EINVAL.  Its
 *                        contents before and after the call mean nothing; it must
 *                        stay untouched until the call's work on the stream is done
 *   work                 one device word, 0 at launch, 0 between the call's two
 *                        launches and left at 0: oth_rollout's contract
 * Every check answers before anything is launched, for n == 0 too.  n == 0 with
 * valid arguments: OTH_OK, nothing launched.
 * OTH_PLAY_BLOCKS in the environment (read per launch) caps both grids, from 1
 * to the resident count; results do not depend on it. */
int othx_play(const uint64_t* start, const uint8_t* start_turn, uint64_t seed, uint64_t game_id0,
              const int8_t* weights_a, const int8_t* weights_b, int depth_a, int depth_b, uint32_t budget_a,
              uint32_t budget_b, int solve_empties, int order, int n_rand_a, int n_rand_b, int swap_colours,
              uint32_t node_limit, uint8_t* a_black, uint64_t* final_boards, int8_t* diff, uint8_t* plies,
              uint8_t* moves, uint8_t* status, uint64_t* nodes, int64_t* hist, void* scratch, int64_t scratch_bytes,
              uint64_t* work, int64_t n, void* stream);

/* bytes of scratch a call of n games needs: OTHX_COUNTER_BYTES + n *
 * OTHX_PARKED_BYTES; OTH_EINVAL for n < 0 */
int64_t othx_scratch_bytes(int64_t n);

/* blocks the first launch of n games uses (no launch; cf. othp_play_grid);
 * order 0 or 1, budgeted 0 or 1, else OTH_EINVAL */
int othx_play_grid(int64_t n, int order, int budgeted);

#ifdef __cplusplus
}
#endif
#endif
