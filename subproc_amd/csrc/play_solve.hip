// play_solve.hip — search self-play whose last plies are the exact solver's,
// for gfx950 (include/othello_play_solve.h).
//
// Two machines, two launches.  A wave whose lanes stood in the search's machine
// and in the solver's would execute both per step and hold both stacks (15.9 KB
// of search frames and 19.25 KB of solver frames per one-wave block), so a game
// changes kernels where it changes machines:
//   * park_*_games: play.hip's and budget.hip's persistent loop, game_loop.hpp's
//     game_body<>, around play_core.hpp's advance() / budget_core.hpp's
//     advance_play() with their kPark flag set.  A game whose turn begins inside the zone (at most
//     solve_empties empty squares; its start included) comes back as
//     othp::kParked: its record (play_solve_core.hpp's pack(): 48 B, three
//     16-byte stores) goes to the slot one atomic on the list's counter names.
//     Games that end above the zone are emitted as they always were.
//   * finish_parked_games: line.hip's solver loop (one-wave blocks, the
//     solver's frames in LDS indexed [depth][field][lane]) over the list.  The
//     count is read on the device, and with it the total that
//     device_common.hpp's take() resets the work word at.  A lane plays its
//     game to the end with play_solve_core.hpp's advance(); moves go to the
//     game's row, the outputs are game_loop.hpp's.
// The counter is zeroed by a memset node in front of the first launch; the two
// launches are ordered by the stream, which makes the first one's stores
// visible to the second.  The slots are handed out in whatever order the lanes
// arrive: nothing depends on it, every game writes its own rows.
//
// Bounds: the first phase's are play.hip's and budget.hip's.  In the second, a
// solve is bounded by node_limit (solve_core.hpp), a game by its plies (at most
// 12 placements and the passes between them; step() stops at 255 whatever the
// boards), a lane by the list and one failing request.  A slot index is below n
// (a game parks once), a record's game index is the one the first phase wrote.
//
// Geometry: one wave per block in both.  First phase: play.hip's 16.1 KB of
// LDS.  Second: 11 frames x 28 B x 64 lanes = 19.25 KB and nothing else, eight
// blocks in a CU's 160 KB (two waves per SIMD).
#include "../../include/othello_budget.h"
#include "../../include/othello_order.h"
#include "../../include/othello_play.h"
#include "../../include/othello_play_solve.h"
#include "../../include/othello_search.h"
#include "../../include/othello_solve.h"
#include "device_common.hpp"
#include "budget_core.hpp"
#include "game_loop.hpp"
#include "play_solve_core.hpp"

static_assert(OTHS_MAX_EMPTIES == oths::kMaxEmpties && OTHM_MAX_DEPTH == othm::kMaxDepth &&
                  OTHM_SEARCHED == othm::kSearched && OTHM_INVALID == othm::kInvalid && OTHM_LIMIT == othm::kLimit &&
                  OTH_PASS == othp::kPassMove && OTHS_DEFAULT_NODE_LIMIT == OTHM_DEFAULT_NODE_LIMIT,
              "header and core disagree");
static_assert(OTHP_MAX_RANDOM == othp::kMaxBudget && OTHP_MAX_PLIES == othp::kMaxPlies &&
                  OTH_MOVES_STRIDE == othp::kMovesStride && OTH_MOVES_STRIDE % 16 == 0 &&
                  OTH_EVAL_WEIGHTS == othm::kEvalPhases * othm::kEvalFeatures,
              "header and core disagree");
static_assert(OTHX_PARKED_BYTES == othx::kRecordWords * 8 && OTHX_COUNTER_BYTES == othx::kCounterWords * 8 &&
                  OTHX_PARKED_BYTES % 16 == 0 && OTHX_COUNTER_BYTES % 16 == 0,
              "header and core disagree");
static_assert(othp::kParked != othm::kSearched && othp::kParked != othm::kInvalid && othp::kParked != othm::kLimit,
              "a parked game is none of the ended ones");

namespace {

using othm::u32;
using othm::u64;

constexpr int kBlock = 64;  // one wave
using othd::DeviceRules;
using othd::kRefillMin;
using othd::status_of;
using SolveStack = othd::LdsStack7<kBlock>;
static_assert(othd::LdsStack9<kBlock>::kFields == othm::kFields && SolveStack::kFields == oths::kFields,
              "the frames' words");

// both phases' arguments: othp_play's outputs by game_loop.hpp's names, and the
// parked list (its counter, then its records)
struct ZoneArgs {
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
    unsigned long long* parked;  // the list's counter
    u64* records;                // othx::kRecordWords words per parked game
    u64 n;
    u64 total;  // the first phase: n + lanes of the grid, what the launch's requests add up to
    u64 seed_state;
    u64 game_id0;
    othp::Match match;  // exact_empties holds solve_empties: the first phase's parking line
    othb::Budgets budgets;
    int8_t w[2][OTH_EVAL_WEIGHTS];  // A's table, B's table
};

using othp::emit;
using othp::MoveRecord;

// game g leaves the first phase for the second
struct Park {
    __device__ __forceinline__ void operator()(const ZoneArgs& a, u64 g, const othp::Game& G) const {
        u64 w[othx::kRecordWords];
        othx::pack(G, g, w);
        const u64 slot = atomicAdd(a.parked, 1ull);
        if (slot >= a.n) return;  // (a game parks once, so never: the check keeps a defect inside the list)
        ulonglong2* r = reinterpret_cast<ulonglong2*>(a.records + slot * othx::kRecordWords);
        r[0] = make_ulonglong2(w[0], w[1]);
        r[1] = make_ulonglong2(w[2], w[3]);
        r[2] = make_ulonglong2(w[4], w[5]);
    }
};

// THE FIRST PHASE: game_loop.hpp's loop with the parking step, by fixed depth or
// by node budget (kBudget), either move order (kOrdered)
__global__ __launch_bounds__(kBlock) void park_fixed_games(ZoneArgs a) {
    othp::game_body<kBlock, false, false, true>(a, Park{});
}
__global__ __launch_bounds__(kBlock) void park_ordered_games(ZoneArgs a) {
    othp::game_body<kBlock, true, false, true>(a, Park{});
}
__global__ __launch_bounds__(kBlock) void park_budget_games(ZoneArgs a) {
    othp::game_body<kBlock, false, true, true>(a, Park{});
}
__global__ __launch_bounds__(kBlock) void park_budget_ordered_games(ZoneArgs a) {
    othp::game_body<kBlock, true, true, true>(a, Park{});
}

// THE SECOND PHASE: the parked games, each played to its end by the solver
__global__ __launch_bounds__(kBlock) void finish_parked_games(ZoneArgs a) {
    __shared__ u32 frames[oths::kFrames * oths::kFields * kBlock];
    const u32 lane = threadIdx.x;
    // (the counter cannot pass n; the bound keeps a defect inside the list)
    const u64 parked = *a.parked;
    const u64 n = parked < a.n ? parked : a.n;
    const u64 total = n + (u64)gridDim.x * kBlock;  // what the launch's requests add up to
    SolveStack stk{frames + lane};
    oths::Lane L;
    L.depth = -1;
    othp::Game G;
    G.live = false;
    MoveRecord rec{nullptr};
    u64 idx = 0;
    bool exhausted = false;  // the lane has made its failing request
    for (;;) {
        const bool idle = !G.live;
        const bool want = idle && !exhausted;
        const u64 wantm = __ballot(want);
        const u64 busym = __ballot(!idle);
        if ((wantm | busym) == 0) break;
        const u64 cnt = (u64)__popcll(wantm);
        if (wantm != 0 && ((int)cnt >= kRefillMin || busym == 0)) {
            const u64 s = othd::take(a.work, total, wantm, cnt, lane);
            if (want) {
                if (s >= n) {
                    exhausted = true;
                } else {
                    const ulonglong2* r = reinterpret_cast<const ulonglong2*>(a.records + s * othx::kRecordWords);
                    const ulonglong2 r0 = r[0], r1 = r[1], r2 = r[2];
                    const u64 w[othx::kRecordWords] = {r0.x, r0.y, r1.x, r1.y, r2.x, r2.y};
                    const u64 g = othx::unpack(G, w);
                    L.depth = -1;
                    if (g >= a.n) {  // (the first phase wrote it: never)
                        G.live = false;
                    } else {
                        idx = g;
                        rec.row = a.moves ? a.moves + g * OTH_MOVES_STRIDE : nullptr;  // (padded by the first phase)
                    }
                }
            }
        }
        if (G.live) {
            othx::advance<DeviceRules>(G, L, stk, a.match.limit, rec);
            if (!G.live) emit(a, idx, G);
        }
    }
}

// one cache per kernel: the first phase's [budgeted][order], then the second's
othd::ResidentBlocks g_resident_park[2][2];
othd::ResidentBlocks g_resident_finish;

const void* park_kernel_of(int order, int budgeted) {
    return budgeted ? (order ? reinterpret_cast<const void*>(park_budget_ordered_games)
                             : reinterpret_cast<const void*>(park_budget_games))
                    : (order ? reinterpret_cast<const void*>(park_ordered_games)
                             : reinterpret_cast<const void*>(park_fixed_games));
}

int park_grid(int64_t n, int order, int budgeted) {
    return othd::launch_grid(g_resident_park[budgeted][order], park_kernel_of(order, budgeted), kBlock, n,
                             "OTH_PLAY_BLOCKS");
}

// the host cannot know the parked count: sized for n
int finish_grid(int64_t n) {
    return othd::launch_grid(g_resident_finish, reinterpret_cast<const void*>(finish_parked_games), kBlock, n,
                             "OTH_PLAY_BLOCKS");
}

}  // namespace

extern "C" {

int64_t othx_scratch_bytes(int64_t n) {
    if (n < 0 || n > (INT64_MAX - OTHX_COUNTER_BYTES) / OTHX_PARKED_BYTES) return OTH_EINVAL;
    return OTHX_COUNTER_BYTES + n * (int64_t)OTHX_PARKED_BYTES;
}

int othx_play(const uint64_t* start, const uint8_t* start_turn, uint64_t seed, uint64_t game_id0,
              const int8_t* weights_a, const int8_t* weights_b, int depth_a, int depth_b, uint32_t budget_a,
              uint32_t budget_b, int solve_empties, int order, int n_rand_a, int n_rand_b, int swap_colours,
              uint32_t node_limit, uint8_t* a_black, uint64_t* final_boards, int8_t* diff, uint8_t* plies,
              uint8_t* moves, uint8_t* status, uint64_t* nodes, int64_t* hist, void* scratch, int64_t scratch_bytes,
              uint64_t* work, int64_t n, void* stream) {
    if (!othp::game_args_ok(order, n, work, weights_a, weights_b, depth_a, depth_b, n_rand_a, n_rand_b) ||
        (budget_a == 0) != (budget_b == 0) || solve_empties < 1 || solve_empties > OTHS_MAX_EMPTIES)
        return OTH_EINVAL;
    const int64_t need = othx_scratch_bytes(n);
    if (need < 0 || !scratch || ((uintptr_t)scratch & 15) || scratch_bytes < need) return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    const int budgeted = budget_a != 0;
    const int grid1 = park_grid(n, order, budgeted);
    const int grid2 = finish_grid(n);
    if (grid1 <= 0 || grid2 <= 0) return status_of(hipErrorInvalidDevice);
    ZoneArgs a;
    othp::fill_game(a, start, start_turn, seed, game_id0, weights_a, weights_b, depth_a, depth_b, solve_empties,
                    n_rand_a, n_rand_b, swap_colours, node_limit, a_black, final_boards, diff, plies, moves, status,
                    nodes, hist, work, n, (int64_t)grid1 * kBlock);
    a.parked = reinterpret_cast<unsigned long long*>(scratch);
    a.records = reinterpret_cast<u64*>(scratch) + othx::kCounterWords;
    a.budgets.budget[0] = budget_a;
    a.budgets.budget[1] = budget_b;
    hipStream_t q = (hipStream_t)stream;
    int rc = status_of(hipMemsetAsync(a.parked, 0, OTHX_COUNTER_BYTES, q));
    if (rc != OTH_OK) return rc;
    if (budgeted) {
        if (order)
            park_budget_ordered_games<<<(unsigned)grid1, kBlock, 0, q>>>(a);
        else
            park_budget_games<<<(unsigned)grid1, kBlock, 0, q>>>(a);
    } else {
        if (order)
            park_ordered_games<<<(unsigned)grid1, kBlock, 0, q>>>(a);
        else
            park_fixed_games<<<(unsigned)grid1, kBlock, 0, q>>>(a);
    }
    rc = status_of(hipGetLastError());
    if (rc != OTH_OK) return rc;
    finish_parked_games<<<(unsigned)grid2, kBlock, 0, q>>>(a);
    return status_of(hipGetLastError());
}

int othx_play_grid(int64_t n, int order, int budgeted) {
    if (order < 0 || order > OTHO_MAX_ORDER || budgeted < 0 || budgeted > 1) return OTH_EINVAL;
    return othd::grid_answer(n, [&] { return park_grid(n, order, budgeted); });
}

}  // extern "C"
