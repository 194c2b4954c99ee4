// search.hip — depth-limited alpha-beta search with the learner's eval at the
// horizon, for gfx950: one lane per position (include/othello_search.h).
//
// The search itself is search_core.hpp's advance(): the solver's one-step
// state machine with a depth horizon.  This file gives it what solve.hip gives
// the solver's, in the same shape:
//   * the rules: bitboard.hpp's moves() and flips_carry();
//   * the stack: an LDS array indexed [depth][field][lane] in 32-bit words (one
//     word per bank whatever depth each lane is at); no per-thread array, no
//     recursion, no scratch;
//   * the eval table: oth_eval's int8 [4][9], passed by value with the launch
//     and widened into LDS (int rows padded to 12) by the block's one wave;
//   * the refill: idle lanes take the next positions from the caller's work
//     word, kRefillMin of them at a time, by device_common.hpp's take()
//     (solve.hip's header has the measurement behind the 8).
//
// search_ordered_kernel is the same loop around order_core.hpp's
// advance_ordered() (include/othello_order.h, order = 1): the lane's scoring
// state is three registers beside its Lane, the frames are the same 9 words.
// Both kernels are instances of search_body<>; order 0 launches search_kernel.
//
// Geometry: one wave per block.  7 frames x 36 B x 64 lanes + the table =
// 15.9 KB of LDS per block, eight blocks in a CU's 160 KB (two waves per
// SIMD).  The waves share nothing; the one barrier orders the table's fill.
#include "../../include/othello_search.h"
#include "../../include/othello_order.h"
#include "device_common.hpp"
#include "order_core.hpp"
#include "search_core.hpp"

static_assert(OTHM_MAX_DEPTH == othm::kMaxDepth && OTHM_TERMINAL_SCALE == othm::kTerminal, "header and core disagree");
static_assert(OTHM_SEARCHED == othm::kSearched && OTHM_INVALID == othm::kInvalid && OTHM_LIMIT == othm::kLimit &&
                  OTHM_NO_MOVE == othm::kNoMove && OTH_PASS == othm::kPassMove,
              "header and core disagree");
static_assert(OTH_EVAL_PHASES == othm::kEvalPhases && OTH_EVAL_FEATURES == othm::kEvalFeatures &&
                  OTH_EVAL_WEIGHTS == othm::kEvalPhases * othm::kEvalFeatures,
              "the eval table's shape");

namespace {

using othm::u32;
using othm::u64;

constexpr int kSearchBlock = 64;  // one wave
using othd::DeviceRules;
using othd::kRefillMin;
using othd::status_of;
using LdsStack = othd::LdsStack9<kSearchBlock>;
static_assert(LdsStack::kFields == othm::kFields, "the frame's words");

struct SearchArgs {
    const u64* boards;
    const uint8_t* turn;
    int32_t* value;
    uint8_t* best_move;
    uint8_t* status;
    u32* nodes;
    unsigned long long* work;
    u64 n;
    u64 total;  // n + lanes of the grid: what the launch's requests add up to
    u32 limit;
    int depth;
    int8_t w[OTH_EVAL_WEIGHTS];
};

__device__ __forceinline__ void emit(const SearchArgs& a, u64 i, int value, u32 mv, u32 status, u32 nodes) {
    if (a.value) a.value[i] = value;
    if (a.best_move) a.best_move[i] = (uint8_t)mv;
    if (a.status) a.status[i] = (uint8_t)status;
    if (a.nodes) a.nodes[i] = nodes;
}

// the persistent loop of both kernels; kOrdered: order_core.hpp's machine
template <bool kOrdered>
__device__ __forceinline__ void search_body(const SearchArgs& a) {
    __shared__ u32 frames[othm::kFrames * othm::kFields * kSearchBlock];
    __shared__ int table[othm::kEvalTable];
    const u32 lane = threadIdx.x;
    if (lane < (u32)othm::kEvalTable) othm::widen_weight(a.w, (int)lane, table);
    __syncthreads();
    LdsStack stk{frames + lane};
    othm::Lane L;
    L.depth = -1;
    othm::Order Q;  // (unused, and gone, when !kOrdered)
    othm::order_reset(Q);
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
                        emit(a, g, 0, othm::kNoMove, othm::kInvalid, 0u);
                    } else {
                        othm::start(L, white ? b.y : b.x, white ? b.x : b.y, a.depth);
                        othm::order_reset(Q);
                        idx = g;
                    }
                }
            }
        }
        if (L.depth >= 0) {
            if constexpr (kOrdered)
                othm::advance_ordered<DeviceRules, true>(L, Q, stk, table, a.limit);
            else
                othm::advance<DeviceRules>(L, stk, table, a.limit);
            if (L.depth < 0) emit(a, idx, L.value, L.best_mv, L.status, L.nodes);
        }
    }
}

__global__ __launch_bounds__(kSearchBlock) void search_kernel(SearchArgs a) { search_body<false>(a); }
__global__ __launch_bounds__(kSearchBlock) void search_ordered_kernel(SearchArgs a) { search_body<true>(a); }

// one cache for search_kernel (order 0), one for the ordered kernel (1)
othd::ResidentBlocks g_resident[2];

int search_grid(int64_t n, int order) {
    const void* kernel = order ? reinterpret_cast<const void*>(search_ordered_kernel)
                               : reinterpret_cast<const void*>(search_kernel);
    return othd::launch_grid(g_resident[order], kernel, kSearchBlock, n, "OTH_SEARCH_BLOCKS");
}

}  // namespace

extern "C" {

int otho_search_ordered(const uint64_t* boards, const uint8_t* turn, int depth, int order, const int8_t* weights,
                        uint32_t node_limit, int32_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
                        uint64_t* work, int64_t n, void* stream) {
    if (order < 0 || order > OTHO_MAX_ORDER) return OTH_EINVAL;
    if (n < 0 || !work || !weights || depth < 1 || depth > OTHM_MAX_DEPTH || (n > 0 && !boards)) return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    const int grid = search_grid(n, order);
    if (grid <= 0) return status_of(hipErrorInvalidDevice);
    SearchArgs a;
    a.boards = boards;
    a.turn = turn;
    a.value = value;
    a.best_move = best_move;
    a.status = status;
    a.nodes = nodes;
    a.work = reinterpret_cast<unsigned long long*>(work);
    a.n = (u64)n;
    a.total = (u64)n + (u64)grid * kSearchBlock;
    a.limit = node_limit ? node_limit : OTHM_DEFAULT_NODE_LIMIT;
    a.depth = depth;
    for (int k = 0; k < OTH_EVAL_WEIGHTS; k++) a.w[k] = weights[k];
    if (order)
        search_ordered_kernel<<<(unsigned)grid, kSearchBlock, 0, (hipStream_t)stream>>>(a);
    else
        search_kernel<<<(unsigned)grid, kSearchBlock, 0, (hipStream_t)stream>>>(a);
    return status_of(hipGetLastError());
}

int othm_search(const uint64_t* boards, const uint8_t* turn, int depth, const int8_t* weights, uint32_t node_limit,
                int32_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes, uint64_t* work, int64_t n,
                void* stream) {
    return otho_search_ordered(boards, turn, depth, 0, weights, node_limit, value, best_move, status, nodes, work, n,
                               stream);
}

int otho_search_ordered_grid(int64_t n, int order) {
    if (order < 0 || order > OTHO_MAX_ORDER) return OTH_EINVAL;
    return othd::grid_answer(n, [&] { return search_grid(n, order); });
}

int othm_search_grid(int64_t n) { return otho_search_ordered_grid(n, 0); }

}  // extern "C"
