// budget.hip — search by node budget for gfx950 (include/othello_budget.h):
// iterative deepening with the fixed-depth search's machine, one lane per
// position (budget_deepen_kernel) or per game (budget_play_kernel).  (The
// position kernel is not named after the search: tests/test_search_abi.py finds
// search.hip's kernel by that name's text.)
//
// budget_core.hpp's deepening layer sits where play_core.hpp's advance() puts
// step(): a lane whose iteration has ended is restarted one ply deeper with what
// is left of its budget, or retired with the deepest completed iteration's
// answer.  The iterations are search_core.hpp's advance() (order_core.hpp's
// advance_ordered() in the *_ordered instances), unchanged, with the lane's own
// limit in a register.  This file gives the layer what search.hip and play.hip
// give the search and the games, in the same shape:
//   * the rules, the LDS stack [depth][field][lane], the widened eval table(s)
//     in LDS, one-wave blocks and a persistent loop;
//   * the refill through the caller's work word at kRefillMin idle lanes
//     (device_common.hpp's take());
//   * per lane, in registers: the root's boards (the search kernel; a game has
//     them already) and budget_core.hpp's Deepen (7 words).
//
// Bounds: an iteration counts at most rem nodes and completed iterations take
// their nodes off rem, so a position costs at most its budget plus the nodes of
// the one iteration that ran into the limit, itself at most the budget: 2 B
// node steps and a constant number of others per node.  A game is bounded by
// its plies times that, and by node_limit for the searches without a budget.
//
// Geometry: search.hip's and play.hip's.  7 frames x 36 B x 64 lanes + the
// table(s): 15.9 KB / 16.1 KB of LDS per block, eight blocks in a CU's 160 KB.
#include "../../include/othello_budget.h"
#include "../../include/othello_order.h"
#include "../../include/othello_play.h"
#include "../../include/othello_search.h"
#include "device_common.hpp"
#include "budget_core.hpp"
#include "game_loop.hpp"

static_assert(OTHM_MAX_DEPTH == othm::kMaxDepth && OTHM_SEARCHED == othm::kSearched &&
                  OTHM_INVALID == othm::kInvalid && OTHM_LIMIT == othm::kLimit && OTHM_NO_MOVE == othm::kNoMove &&
                  OTH_PASS == othp::kPassMove,
              "header and core disagree");
static_assert(OTHP_MAX_RANDOM == othp::kMaxBudget && OTH_MOVES_STRIDE == othp::kMovesStride &&
                  OTH_MOVES_STRIDE % 16 == 0 && OTH_EVAL_WEIGHTS == othm::kEvalPhases * othm::kEvalFeatures,
              "header and core disagree");

namespace {

using othm::u32;
using othm::u64;

constexpr int kBudgetBlock = 64;  // one wave
using othd::DeviceRules;
using othd::kRefillMin;
using othd::status_of;
using LdsStack = othd::LdsStack9<kBudgetBlock>;
static_assert(LdsStack::kFields == othm::kFields, "the frame's words");

struct BudgetSearchArgs {
    const u64* boards;
    const uint8_t* turn;
    const u32* budgets;  // NULL: `budget` everywhere
    int32_t* value;
    uint8_t* best_move;
    uint8_t* depth;
    uint8_t* status;
    u32* nodes;
    unsigned long long* work;
    u64 n;
    u64 total;  // n + lanes of the grid: what the launch's requests add up to
    u32 budget;
    int cap;
    int8_t w[OTH_EVAL_WEIGHTS];
};

__device__ __forceinline__ void emit(const BudgetSearchArgs& a, u64 i, int value, u32 mv, u32 depth, u32 status,
                                     u32 nodes) {
    if (a.value) a.value[i] = value;
    if (a.best_move) a.best_move[i] = (uint8_t)mv;
    if (a.depth) a.depth[i] = (uint8_t)depth;
    if (a.status) a.status[i] = (uint8_t)status;
    if (a.nodes) a.nodes[i] = nodes;
}

// the persistent loop of both search kernels; kOrdered: order_core.hpp's machine
template <bool kOrdered>
__device__ __forceinline__ void budget_search_body(const BudgetSearchArgs& a) {
    __shared__ u32 frames[othm::kFrames * othm::kFields * kBudgetBlock];
    __shared__ int table[othm::kEvalTable];
    const u32 lane = threadIdx.x;
    if (lane < (u32)othm::kEvalTable) othm::widen_weight(a.w, (int)lane, table);
    __syncthreads();
    LdsStack stk{frames + lane};
    othm::Lane L;
    L.depth = -1;
    othm::Order Q;  // (unused, and gone, when !kOrdered)
    othm::order_reset(Q);
    othb::Deepen D;
    u64 P = 0, O = 0;  // the lane's root: the mover's discs, the other side's
    u64 idx = 0;
    bool exhausted = false;  // the lane has made its failing request
    for (;;) {
        const bool idle = L.depth < 0;
        const bool want = idle && !exhausted;
        const u64 wantm = __ballot(want);
        const u64 busym = __ballot(!idle);
        if ((wantm | busym) == 0) break;
        const u64 cnt = (u64)__popcll(wantm);
        if (wantm != 0 && ((int)cnt >= kRefillMin || busym == 0)) {
            const u64 g = othd::take(a.work, a.total, wantm, cnt, lane);
            if (want) {
                if (g >= a.n) {
                    exhausted = true;
                } else {
                    const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.boards)[g];
                    const bool white = a.turn && a.turn[g] == OTH_WHITE;
                    if (b.x & b.y) {
                        emit(a, g, 0, othm::kNoMove, 0u, othm::kInvalid, 0u);
                    } else {
                        P = white ? b.y : b.x;
                        O = white ? b.x : b.y;
                        othb::begin_search<DeviceRules>(D, L, P, O, a.budgets ? a.budgets[g] : a.budget, a.cap);
                        othm::order_reset(Q);
                        idx = g;
                        if (L.depth < 0) emit(a, g, 0, othm::kNoMove, 0u, othm::kLimit, 0u);  // a budget of 0
                    }
                }
            }
        }
        if (L.depth >= 0 && othb::advance_search<DeviceRules, kOrdered>(D, L, Q, stk, table, P, O))
            emit(a, idx, D.value, D.move, D.depth, othb::status_of(D), D.nodes);
    }
}

__global__ __launch_bounds__(kBudgetBlock) void budget_deepen_kernel(BudgetSearchArgs a) {
    budget_search_body<false>(a);
}
__global__ __launch_bounds__(kBudgetBlock) void budget_deepen_ordered_kernel(BudgetSearchArgs a) {
    budget_search_body<true>(a);
}

struct BudgetPlayArgs {
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
    othb::Budgets budgets;
    int8_t w[2][OTH_EVAL_WEIGHTS];  // A's table, B's table
};

// the persistent loop of both game kernels is game_loop.hpp's, by budget and
// without a parking step
__global__ __launch_bounds__(kBudgetBlock) void budget_play_kernel(BudgetPlayArgs a) {
    othp::game_body<kBudgetBlock, false, true>(a);
}
__global__ __launch_bounds__(kBudgetBlock) void budget_play_ordered_kernel(BudgetPlayArgs a) {
    othp::game_body<kBudgetBlock, true, true>(a);
}

// one cache per kernel: [0] the searches, [1] the games; order 0, then 1
othd::ResidentBlocks g_resident[2][2];

int grid_of(int64_t n, int play, int order) {
    const void* kernel =
        play ? (order ? reinterpret_cast<const void*>(budget_play_ordered_kernel)
                      : reinterpret_cast<const void*>(budget_play_kernel))
             : (order ? reinterpret_cast<const void*>(budget_deepen_ordered_kernel)
                      : reinterpret_cast<const void*>(budget_deepen_kernel));
    return othd::launch_grid(g_resident[play][order], kernel, kBudgetBlock, n, "OTH_BUDGET_BLOCKS");
}

}  // namespace

extern "C" {

int othb_search(const uint64_t* boards, const uint8_t* turn, int max_depth, const int8_t* weights, uint32_t budget,
                const uint32_t* budgets, int order, int32_t* value, uint8_t* best_move, uint8_t* depth,
                uint8_t* status, uint32_t* nodes, uint64_t* work, int64_t n, void* stream) {
    if (order < 0 || order > OTHO_MAX_ORDER) return OTH_EINVAL;
    if (n < 0 || !work || !weights || max_depth < 1 || max_depth > OTHM_MAX_DEPTH || (n > 0 && !boards) ||
        (!budgets && budget == 0))
        return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    const int grid = grid_of(n, 0, order);
    if (grid <= 0) return status_of(hipErrorInvalidDevice);
    BudgetSearchArgs a;
    a.boards = boards;
    a.turn = turn;
    a.budgets = budgets;
    a.value = value;
    a.best_move = best_move;
    a.depth = depth;
    a.status = status;
    a.nodes = nodes;
    a.work = reinterpret_cast<unsigned long long*>(work);
    a.n = (u64)n;
    a.total = (u64)n + (u64)grid * kBudgetBlock;
    a.budget = budget;
    a.cap = max_depth;
    for (int k = 0; k < OTH_EVAL_WEIGHTS; k++) a.w[k] = weights[k];
    if (order)
        budget_deepen_ordered_kernel<<<(unsigned)grid, kBudgetBlock, 0, (hipStream_t)stream>>>(a);
    else
        budget_deepen_kernel<<<(unsigned)grid, kBudgetBlock, 0, (hipStream_t)stream>>>(a);
    return status_of(hipGetLastError());
}

int othb_play(const uint64_t* start, const uint8_t* start_turn, uint64_t seed, uint64_t game_id0,
              const int8_t* weights_a, const int8_t* weights_b, int depth_a, int depth_b, uint32_t budget_a,
              uint32_t budget_b, int exact_empties, int order, int n_rand_a, int n_rand_b, int swap_colours,
              uint32_t node_limit, uint8_t* a_black, uint64_t* final_boards, int8_t* diff, uint8_t* plies,
              uint8_t* moves, uint8_t* status, uint64_t* nodes, int64_t* hist, uint64_t* work, int64_t n,
              void* stream) {
    if (!othp::game_args_ok(order, n, work, weights_a, weights_b, depth_a, depth_b, n_rand_a, n_rand_b) ||
        budget_a == 0 || budget_b == 0 || exact_empties < 0 || exact_empties > OTHM_MAX_DEPTH)
        return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    const int grid = grid_of(n, 1, order);
    if (grid <= 0) return status_of(hipErrorInvalidDevice);
    BudgetPlayArgs a;
    othp::fill_game(a, start, start_turn, seed, game_id0, weights_a, weights_b, depth_a, depth_b, exact_empties,
                    n_rand_a, n_rand_b, swap_colours, node_limit, a_black, final_boards, diff, plies, moves, status,
                    nodes, hist, work, n, (int64_t)grid * kBudgetBlock);
    a.budgets.budget[0] = budget_a;
    a.budgets.budget[1] = budget_b;
    if (order)
        budget_play_ordered_kernel<<<(unsigned)grid, kBudgetBlock, 0, (hipStream_t)stream>>>(a);
    else
        budget_play_kernel<<<(unsigned)grid, kBudgetBlock, 0, (hipStream_t)stream>>>(a);
    return status_of(hipGetLastError());
}

int othb_search_grid(int64_t n) {
    return othd::grid_answer(n, [&] { return grid_of(n, 0, 0); });
}

int othb_play_grid(int64_t n) {
    return othd::grid_answer(n, [&] { return grid_of(n, 1, 0); });
}

}  // extern "C"
