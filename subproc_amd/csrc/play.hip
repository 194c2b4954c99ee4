// play.hip — search self-play for gfx950: whole games between two searching
// players in one launch, one lane per game (include/othello_play.h).
//
// A lane's search is search_core.hpp's advance(), unchanged; play_core.hpp's
// step() is the transition that takes a lane from a finished root to the next
// one: play the move, record it, settle game over / pass / coin / single move,
// start the new mover's search.  This file gives the two what search.hip gives
// the search, in the same shape:
//   * the rules: bitboard.hpp's moves() and flips_carry();
//   * the stack: an LDS array indexed [depth][field][lane] in 32-bit words; no
//     per-thread array, no recursion, no scratch;
//   * both players' eval tables, passed by value with the launch and widened
//     into LDS (2 x 48 ints) by the block's one wave; a lane's search reads the
//     table of its mover;
//   * the refill: idle lanes take the next GAMES from the caller's work word,
//     kRefillMin of them at a time: device_common.hpp's take() at game
//     granularity.
// The game's state (boards, ply, LCG state and increment, the two budgets, the
// colour bits, the game index, the node sum) stays in registers.  Move bytes
// and the per-game outputs are plain vector stores; the histogram is three
// global atomics per finished game.
//
// play_ordered_kernel is the same loop with order_core.hpp's ordered search
// inside (include/othello_order.h, order = 1; play_core.hpp's advance() with
// its flag set); both kernels are instances of game_loop.hpp's game_body<>,
// which budget.hip's and play_solve.hip's game kernels are too.
//
// Bounds: a lane's loop ends.  Every search is bounded by node_limit (at most
// that many steps that count a node, a constant number of others per node);
// every game by its plies (60 placements and the passes between them; step()
// stops a game at 255 whatever its boards); every lane by the games of the
// launch and one failing request.
//
// Geometry: one wave per block.  7 frames x 36 B x 64 lanes + the tables =
// 16.1 KB of LDS per block, eight blocks in a CU's 160 KB (two waves per SIMD).
#include "../../include/othello_play.h"
#include "../../include/othello_search.h"
#include "../../include/othello_order.h"
#include "device_common.hpp"
#include "game_loop.hpp"
#include "play_core.hpp"

static_assert(OTHM_MAX_DEPTH == othm::kMaxDepth && OTHM_SEARCHED == othm::kSearched &&
                  OTHM_INVALID == othm::kInvalid && OTHM_LIMIT == othm::kLimit && OTH_PASS == othp::kPassMove,
              "header and core disagree");
static_assert(OTHP_MAX_RANDOM == othp::kMaxBudget && OTHP_MAX_PLIES == othp::kMaxPlies &&
                  OTH_MOVES_STRIDE == othp::kMovesStride && OTH_MOVES_STRIDE % 16 == 0,
              "header and core disagree");
static_assert(OTH_EVAL_WEIGHTS == othm::kEvalPhases * othm::kEvalFeatures, "the eval table's shape");

namespace {

using othm::u32;
using othm::u64;

constexpr int kPlayBlock = 64;  // one wave
using othd::status_of;
static_assert(othd::LdsStack9<kPlayBlock>::kFields == othm::kFields, "the frame's words");

struct PlayArgs {
    const u64* start;
    const uint8_t* start_turn;
    uint8_t* a_black;
    u64* final_boards;
    int8_t* diff;
    uint8_t* plies;
    uint8_t* moves;
    uint8_t* status;
    u64* nodes;
    unsigned long long* hist;
    unsigned long long* work;
    u64 n;
    u64 total;  // n + lanes of the grid: what the launch's requests add up to
    u64 seed_state;
    u64 game_id0;
    othp::Match match;
    int8_t w[2][OTH_EVAL_WEIGHTS];  // A's table, B's table
};

// the persistent loop of both kernels is game_loop.hpp's, by fixed depth and
// without a parking step
__global__ __launch_bounds__(kPlayBlock) void play_kernel(PlayArgs a) {
    othp::game_body<kPlayBlock, false, false>(a);
}
__global__ __launch_bounds__(kPlayBlock) void play_ordered_kernel(PlayArgs a) {
    othp::game_body<kPlayBlock, true, false>(a);
}

// one cache for play_kernel (order 0), one for the ordered kernel (1)
othd::ResidentBlocks g_resident[2];

int play_grid(int64_t n, int order) {
    const void* kernel = order ? reinterpret_cast<const void*>(play_ordered_kernel)
                               : reinterpret_cast<const void*>(play_kernel);
    return othd::launch_grid(g_resident[order], kernel, kPlayBlock, n, "OTH_PLAY_BLOCKS");
}

}  // namespace

extern "C" {

int otho_play_ordered(const uint64_t* start, const uint8_t* start_turn, uint64_t seed, uint64_t game_id0,
                      const int8_t* weights_a, const int8_t* weights_b, int depth_a, int depth_b, int exact_empties,
                      int order, int n_rand_a, int n_rand_b, int swap_colours, uint32_t node_limit, uint8_t* a_black,
                      uint64_t* final_boards, int8_t* diff, uint8_t* plies, uint8_t* moves, uint8_t* status,
                      uint64_t* nodes, int64_t* hist, uint64_t* work, int64_t n, void* stream) {
    if (!othp::game_args_ok(order, n, work, weights_a, weights_b, depth_a, depth_b, n_rand_a, n_rand_b) ||
        exact_empties < 0 || exact_empties > OTHM_MAX_DEPTH)
        return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    const int grid = play_grid(n, order);
    if (grid <= 0) return status_of(hipErrorInvalidDevice);
    PlayArgs a;
    othp::fill_game(a, start, start_turn, seed, game_id0, weights_a, weights_b, depth_a, depth_b, exact_empties,
                    n_rand_a, n_rand_b, swap_colours, node_limit, a_black, final_boards, diff, plies, moves, status,
                    nodes, hist, work, n, (int64_t)grid * kPlayBlock);
    if (order)
        play_ordered_kernel<<<(unsigned)grid, kPlayBlock, 0, (hipStream_t)stream>>>(a);
    else
        play_kernel<<<(unsigned)grid, kPlayBlock, 0, (hipStream_t)stream>>>(a);
    return status_of(hipGetLastError());
}

int othp_play(const uint64_t* start, const uint8_t* start_turn, uint64_t seed, uint64_t game_id0,
              const int8_t* weights_a, const int8_t* weights_b, int depth_a, int depth_b, int exact_empties,
              int n_rand_a, int n_rand_b, int swap_colours, uint32_t node_limit, uint8_t* a_black,
              uint64_t* final_boards, int8_t* diff, uint8_t* plies, uint8_t* moves, uint8_t* status, uint64_t* nodes,
              int64_t* hist, uint64_t* work, int64_t n, void* stream) {
    return otho_play_ordered(start, start_turn, seed, game_id0, weights_a, weights_b, depth_a, depth_b, exact_empties, 0,
                             n_rand_a, n_rand_b, swap_colours, node_limit, a_black, final_boards, diff, plies, moves,
                             status, nodes, hist, work, n, stream);
}

int otho_play_ordered_grid(int64_t n, int order) {
    if (order < 0 || order > OTHO_MAX_ORDER) return OTH_EINVAL;
    return othd::grid_answer(n, [&] { return play_grid(n, order); });
}

int othp_play_grid(int64_t n) { return otho_play_ordered_grid(n, 0); }

}  // extern "C"
