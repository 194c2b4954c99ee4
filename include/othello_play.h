/*
 * othello_play.h — C-ABI of the search self-play of libsubproc_amd_hip.so
 * (subproc_amd/csrc/play.hip, gfx950): whole games between two searching
 * players, one GPU lane per game, every policy move chosen by
 * othello_search.h's depth-limited search.  Conventions as in othello_search.h:
 * boards are 2 x uint64 [black, white], every pointer is DEVICE memory owned by
 * the caller EXCEPT the two weight tables (host), calls are asynchronous on
 * `stream`, allocate nothing, never synchronise, and return OTH_OK, OTH_EINVAL
 * or -(hipError_t).
 *
 * The functions of this header are prefixed othp_ (oth_ is othello.h's set,
 * oths_ the exact solver's, othm_ the search's).
 *
 * The game.  Game i has global id game_id0 + i and draws from that id's counter
 * RNG stream, so results do not depend on how games are split
 * over launches.  It starts from the opening with Black to move (start ==
 * NULL), or from start[i] with White to move if start_turn[i] == 2, else Black
 * (start_turn == NULL: Black everywhere): oth_rollout's rule.
 *
 * Players A and B, colours and random moves are oth_rollout_runner's schedule
 * (othello.h), draw for draw:
 *   - with swap_colours != 0 the game's first draw is c = pick(2) and A plays
 *     White iff c == 1; otherwise A plays Black;
 *   - each player starts with min(n_rand, 10) random moves to place;
 *   - on each of its turns, a pass included, a player with budget r > 0 draws
 *     c = pick(r); if c == 0 and it has a legal move, it plays the legal move
 *     of index pick(#legal) in puttables order and r -= 1.
 * Otherwise the turn is the first of these that applies:
 *   1. neither side can move: the game is over (no draw is made);
 *   2. the mover has no move: it passes (OTH_PASS); the pass is a ply, as in
 *      the rollouts;
 *   3. the mover has exactly one legal move: it is played, without a search;
 *   4. otherwise the move is othm_search's best_move for the position and the
 *      mover, with the mover's table (weights_a / weights_b) and depth
 *      (depth_a / depth_b) -- or, once the position has empties <=
 *      exact_empties empty squares, max(depth, empties) plies, so that the
 *      search reaches the end of the game and the move is the solver's
 *      (othello_search.h, "Value").  node_limit bounds each search (0 =
 *      OTHM_DEFAULT_NODE_LIMIT).
 *
 * status[i]:
 *   OTHM_SEARCHED  the game was played to its end;
 *   OTHM_INVALID   start[i]'s boards overlap: nothing is played and no draw is
 *                  made; a_black 1, final_boards = start[i], diff 0, plies 0,
 *                  nodes 0, the move record all 255; not counted in hist;
 *   OTHM_LIMIT     a search of the game hit node_limit: the game stops at that
 *                  position; final_boards, diff (the disc difference there),
 *                  plies and moves describe the game up to it; not counted in
 *                  hist.  (A game of 255 plies would stop likewise; from
 *                  disjoint boards no game has more than 121.)
 * So the kernel is bounded: every search by node_limit, every game by its
 * plies.
 */
#ifndef SUBPROC_AMD_OTHELLO_PLAY_H
#define SUBPROC_AMD_OTHELLO_PLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTHP_MAX_RANDOM 10 /* the cap of n_rand_a / n_rand_b (GameRunner's N_RAND_HAND_UNTIL) */
#define OTHP_MAX_PLIES 255 /* plies is a byte */

/* Play the n games.
 *   weights_a / weights_b  HOST int8[36] each, oth_eval's tables; copied into
 *                 the launch (NULL: OTH_EINVAL)
 *   depth_a / depth_b      1..OTHM_MAX_DEPTH, else OTH_EINVAL
 *   exact_empties          0..OTHM_MAX_DEPTH, else OTH_EINVAL; 0: never
 *   n_rand_a / n_rand_b    >= 0, else OTH_EINVAL
 * Outputs, each may be NULL; as oth_rollout_runner's where it has them:
 *   a_black      uint8[n]     1 where A played Black
 *   final_boards uint64[n][2] [black, white]
 *   diff         int8[n]      black discs - white discs of final_boards
 *   plies        uint8[n]     moves made, passes included
 *   moves        uint8[n * OTH_MOVES_STRIDE], 16-byte aligned: move codes,
 *                255-padded; plies past the stride are not recorded
 *   status       uint8[n]     OTHM_SEARCHED / INVALID / LIMIT
 *   nodes        uint64[n]    the sum of the game's searches' nodes (the
 *                limited one's included).  A diagnostic: a function of the game,
 *                the arguments and the build only; nothing may compare it
 *                across builds
 *   hist         int64[OTH_HIST_BINS], ACCUMULATED over the OTHM_SEARCHED
 *                games: oth_rollout's bins
 * work: one device word, 0 at launch, left at 0 -- oth_rollout's contract; a
 * stream's launches may share one word between rollouts, solves, searches and
 * these.  n == 0: OTH_OK, nothing launched.
 * OTH_PLAY_BLOCKS in the environment (read per launch) caps the grid, from 1 to
 * the resident count; results do not depend on it.  One lane plays one game, so
 * a launch lasts as long as its longest game. */
int othp_play(const uint64_t* start, const uint8_t* start_turn, uint64_t seed, uint64_t game_id0,
              const int8_t* weights_a, const int8_t* weights_b, int depth_a, int depth_b, int exact_empties,
              int n_rand_a, int n_rand_b, int swap_colours, uint32_t node_limit,
              uint8_t* a_black, uint64_t* final_boards, int8_t* diff, uint8_t* plies, uint8_t* moves,
              uint8_t* status, uint64_t* nodes, int64_t* hist, uint64_t* work, int64_t n, void* stream);

/* blocks a launch of n games uses (no launch; cf. othm_search_grid) */
int othp_play_grid(int64_t n);

#ifdef __cplusplus
}
#endif
#endif
