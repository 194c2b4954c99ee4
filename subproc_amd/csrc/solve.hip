// solve.hip — exact endgame solver for gfx950: batched perfect-play search, one
// lane per position (include/othello_solve.h).
//
// The search itself is solve_core.hpp's advance(): one step of one position's
// alpha-beta per loop iteration, so the 64 lanes of a wave, each somewhere in
// its own tree, execute the same instructions.  This file gives it
//   * the rules: bitboard.hpp's moves() and flips_carry(), the ones the step
//     kernel plays by (no second statement of the rules);
//   * the stack: an LDS array indexed [depth][field][lane] in 32-bit words, so
//     a wave's access is one word per bank whatever depth each lane is at.
//     No per-thread array, no recursion: the kernel uses no scratch;
//   * the refill: a lane whose position ends takes the next one from the
//     caller's work word.  The wave's idle lanes are counted by one ballot per
//     iteration; once kRefillMin of them wait (or nothing else is left to do)
//     they are served by device_common.hpp's take(), which states the word's
//     protocol (oth_rollout's contract: 0 at launch, left at 0).  Measured
//     (DESIGN.md §12, 1M positions at 6 empties / 524k at 8, full grid):
//     refilling each lane at once 12.4 / 47.9 ms (the one work word saturates:
//     an atomic per wave nearly every iteration), at 8 idle lanes 4.7 / 48.4
//     ms, a whole wave at a time like the rollouts 8.9 / 84.4 ms.
//
// Geometry: one wave per block.  11 frames x 28 B x 64 lanes = 19.25 KB of LDS
// per block, eight blocks in a CU's 160 KB: two waves per SIMD, which this
// dependent VALU chain wants (a 256-thread block would be alone on its CU, one
// wave per SIMD).  The waves share nothing, so there is no barrier.
#include "../../include/othello_solve.h"
#include "../../include/othello_solve_window.h"
#include "device_common.hpp"
#include "solve_core.hpp"

static_assert(OTHS_MAX_EMPTIES == oths::kMaxEmpties, "header and core disagree");
static_assert(OTHS_SKIPPED == oths::kSkipped && OTHS_SOLVED == oths::kSolved && OTHS_INVALID == oths::kInvalid &&
                  OTHS_LIMIT == oths::kLimit && OTHS_NO_MOVE == oths::kNoMove && OTH_PASS == oths::kPassMove,
              "header and core disagree");
static_assert(OTHS_BADWINDOW == oths::kBadWindow && OTHW_ALPHA_MIN == -oths::kInf && OTHW_BETA_MAX == oths::kInf,
              "header and core disagree");

namespace {

using oths::u32;
using oths::u64;

constexpr int kSolveBlock = 64;  // one wave
using othd::DeviceRules;
using othd::env_int;
using othd::kRefillMin;
using othd::status_of;
using LdsStack = othd::LdsStack7<kSolveBlock>;
static_assert(LdsStack::kFields == oths::kFields, "the frame's words");

struct SolveArgs {
    const u64* boards;
    const uint8_t* turn;
    int8_t* value;
    uint8_t* best_move;
    uint8_t* status;
    u32* nodes;
    unsigned long long* work;
    u64 n;
    u64 total;  // n + lanes of the grid: what the launch's requests add up to
    u32 limit;
    int max_empties;
    int refill_min;  // idle lanes that make a wave refill (1: each lane at once .. 64: the rollouts' batch dequeue)
    // othw_solve only: each position's root window, NULL = -65 / 65 everywhere
    const int8_t* alpha;
    const int8_t* beta;
};

__device__ __forceinline__ void emit(const SolveArgs& a, u64 i, int value, u32 mv, u32 status, u32 nodes) {
    if (a.value) a.value[i] = (int8_t)value;
    if (a.best_move) a.best_move[i] = (uint8_t)mv;
    if (a.status) a.status[i] = (uint8_t)status;
    if (a.nodes) a.nodes[i] = nodes;
}

// oths_solve's kernel, the text it always was: a.alpha and a.beta are not read.
__global__ __launch_bounds__(kSolveBlock) void solve_kernel(SolveArgs a) {
    __shared__ u32 frames[oths::kFrames * oths::kFields * kSolveBlock];
    const u32 lane = threadIdx.x;
    LdsStack stk{frames + lane};
    oths::Lane L;
    L.depth = -1;
    u64 idx = 0;
    bool exhausted = false;  // the lane has made its failing request
    for (;;) {
        const bool idle = L.depth < 0;
        const bool want = idle && !exhausted;
        const u64 wantm = __ballot(want);
        const u64 busym = __ballot(!idle);
        if ((wantm | busym) == 0) break;
        const u64 cnt = (u64)__popcll(wantm);
        if (wantm != 0 && ((int)cnt >= a.refill_min || busym == 0)) {
            const u64 g = othd::take(a.work, a.total, wantm, cnt, lane);
            if (want) {
                if (g >= a.n) {
                    exhausted = true;
                } else {
                    const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.boards)[g];
                    const bool white = a.turn && a.turn[g] == OTH_WHITE;
                    const u32 st = oths::classify(b.x, b.y, 64 - __popcll(b.x | b.y), a.max_empties);
                    if (st == oths::kSolved) {
                        oths::start(L, white ? b.y : b.x, white ? b.x : b.y);
                        idx = g;
                    } else {
                        emit(a, g, 0, oths::kNoMove, st, 0u);
                    }
                }
            }
        }
        if (L.depth >= 0) {
            oths::advance<DeviceRules>(L, stk, a.limit);
            if (L.depth < 0) emit(a, idx, L.value, L.best_mv, L.status, L.nodes);
        }
    }
}

// othw_solve's kernel: solve_kernel's text with each position's root window,
// read when the lane takes the position and once more when it emits (the
// clamp), so no register holds it through the search.  Written out a second
// time, as solve_tree.hip's task kernels are: a kernel that calls its loop
// compiles to other code than a kernel that is its loop, and solve_kernel's code
// is the build's before (DESIGN.md §20 has the comparison).  A change to one is
// a change to both.
__global__ __launch_bounds__(kSolveBlock) void solve_windowed(SolveArgs a) {
    __shared__ u32 frames[oths::kFrames * oths::kFields * kSolveBlock];
    const u32 lane = threadIdx.x;
    LdsStack stk{frames + lane};
    oths::Lane L;
    L.depth = -1;
    u64 idx = 0;
    bool exhausted = false;  // the lane has made its failing request
    for (;;) {
        const bool idle = L.depth < 0;
        const bool want = idle && !exhausted;
        const u64 wantm = __ballot(want);
        const u64 busym = __ballot(!idle);
        if ((wantm | busym) == 0) break;
        const u64 cnt = (u64)__popcll(wantm);
        if (wantm != 0 && ((int)cnt >= a.refill_min || busym == 0)) {
            const u64 g = othd::take(a.work, a.total, wantm, cnt, lane);
            if (want) {
                if (g >= a.n) {
                    exhausted = true;
                } else {
                    const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.boards)[g];
                    const bool white = a.turn && a.turn[g] == OTH_WHITE;
                    const u32 st = oths::classify(b.x, b.y, 64 - __popcll(b.x | b.y), a.max_empties);
                    const int ra = a.alpha ? (int)a.alpha[g] : -oths::kInf;
                    const int rb = a.beta ? (int)a.beta[g] : oths::kInf;
                    if (st != oths::kSolved) {
                        emit(a, g, 0, oths::kNoMove, st, 0u);
                    } else if (!oths::window_ok(ra, rb)) {
                        emit(a, g, 0, oths::kNoMove, oths::kBadWindow, 0u);
                    } else {
                        oths::start(L, white ? b.y : b.x, white ? b.x : b.y, ra, rb);
                        idx = g;
                    }
                }
            }
        }
        if (L.depth >= 0) {
            oths::advance<DeviceRules>(L, stk, a.limit);
            if (L.depth < 0) {
                if (L.status == oths::kSolved)
                    L.value = oths::clamp_to_window(L.value, a.alpha ? (int)a.alpha[idx] : -oths::kInf,
                                                    a.beta ? (int)a.beta[idx] : oths::kInf);
                emit(a, idx, L.value, L.best_mv, L.status, L.nodes);
            }
        }
    }
}

othd::ResidentBlocks g_resident[2];  // oths_solve's kernel, othw_solve's

int solve_grid(int64_t n, bool window = false) {
    const void* kernel = window ? reinterpret_cast<const void*>(solve_windowed)
                                : reinterpret_cast<const void*>(solve_kernel);
    return othd::launch_grid(g_resident[window ? 1 : 0], kernel, kSolveBlock, n, "OTH_SOLVE_BLOCKS");
}

template <bool kWindow>
int launch_solve(const uint64_t* boards, const uint8_t* turn, const int8_t* alpha, const int8_t* beta, int max_empties,
                 uint32_t node_limit, int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes, uint64_t* work,
                 int64_t n, void* stream) {
    if (n < 0 || !work || max_empties < 0 || max_empties > OTHS_MAX_EMPTIES || (n > 0 && !boards)) return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    const int grid = solve_grid(n, kWindow);
    if (grid <= 0) return status_of(hipErrorInvalidDevice);
    SolveArgs a;
    a.boards = boards;
    a.turn = turn;
    a.value = value;
    a.best_move = best_move;
    a.status = status;
    a.nodes = nodes;
    a.work = reinterpret_cast<unsigned long long*>(work);
    a.n = (u64)n;
    a.total = (u64)n + (u64)grid * kSolveBlock;
    a.limit = node_limit ? node_limit : OTHS_DEFAULT_NODE_LIMIT;
    a.max_empties = max_empties;
    // OTH_SOLVE_REFILL=1..64 (tools/solve_bench.py's A/B): the idle lanes that
    // make a wave refill; 64 is the rollouts' batch dequeue
    a.refill_min = std::min(std::max(env_int("OTH_SOLVE_REFILL", kRefillMin), 1), kSolveBlock);
    a.alpha = alpha;
    a.beta = beta;
    if (kWindow)
        solve_windowed<<<(unsigned)grid, kSolveBlock, 0, (hipStream_t)stream>>>(a);
    else
        solve_kernel<<<(unsigned)grid, kSolveBlock, 0, (hipStream_t)stream>>>(a);
    return status_of(hipGetLastError());
}

}  // namespace

extern "C" {

int oths_solve(const uint64_t* boards, const uint8_t* turn, int max_empties, uint32_t node_limit, int8_t* value,
               uint8_t* best_move, uint8_t* status, uint32_t* nodes, uint64_t* work, int64_t n, void* stream) {
    return launch_solve<false>(boards, turn, nullptr, nullptr, max_empties, node_limit, value, best_move, status, nodes,
                               work, n, stream);
}

int othw_solve(const uint64_t* boards, const uint8_t* turn, const int8_t* alpha, const int8_t* beta, int max_empties,
               uint32_t node_limit, int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes, uint64_t* work,
               int64_t n, void* stream) {
    return launch_solve<true>(boards, turn, alpha, beta, max_empties, node_limit, value, best_move, status, nodes, work,
                              n, stream);
}

int oths_solve_grid(int64_t n) {
    return othd::grid_answer(n, [&] { return solve_grid(n); });
}

}  // extern "C"
