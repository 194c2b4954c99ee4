// line.hip — the principal variation for gfx950 (include/othello_line.h,
// DESIGN.md §24): the line of best play behind a value, one lane per position,
// from the exact solver (line_exact_walk) and from the depth-limited search
// (line_depth_walk, line_depth_ordered_walk).  (The kernels are not named after
// the solver and the search: tests/test_solve_abi.py and tests/test_search_abi.py
// find solve.hip's and search.hip's kernels by those names' text.)
//
// line_core.hpp's layer sits where budget_core.hpp puts deepen(): a lane whose
// search has ended plays the move found and is restarted on the child as a root
// of its own with the window narrowed to (-v - 1, -v + 1), or retired.  The
// searches are solve_core.hpp's advance() and search_core.hpp's advance()
// (order_core.hpp's advance_ordered() in the ordered instance), unchanged.  This
// file gives the layer what solve.hip and search.hip give the machines, in the
// same shape:
//   * the rules, the LDS stack [depth][field][lane], the widened eval table in
//     LDS, one-wave blocks and a persistent loop;
//   * the refill through the caller's work word at kRefillMin idle lanes
//     (device_common.hpp's take());
//   * per lane, in registers: line_core.hpp's Walk (the position the walk
//     stands at, the root's answer, the nodes' sum) and the root's colour.
// The line's bytes go straight to global memory as each move is settled: the
// row is padded with two 16-byte stores when the lane takes the position, a
// move is one byte store per ply of the line (not per node), and a walk that
// ends at a limit pads the row again.
//
// Bounds: a walk makes at most OTHL_LINE_STRIDE searches, each bounded by the
// node limit as in the existing kernels.
//
// Geometry: solve.hip's (11 frames x 28 B x 64 lanes = 19.25 KB of LDS) and
// search.hip's (7 frames x 36 B x 64 lanes + the table = 15.9 KB), eight blocks
// in a CU's 160 KB.
#include "../../include/othello_line.h"
#include "../../include/othello_order.h"
#include "../../include/othello_search.h"
#include "../../include/othello_solve.h"
#include "device_common.hpp"
#include "line_core.hpp"

static_assert(OTHL_LINE_STRIDE == othl::kLineStride && OTHL_LINE_STRIDE % 16 == 0 && OTHL_BADDEPTH == othl::kBadDepth,
              "header and core disagree");
static_assert(OTHL_BADDEPTH != OTHS_SKIPPED && OTHL_BADDEPTH != OTHS_SOLVED && OTHL_BADDEPTH != OTHS_INVALID &&
                  OTHL_BADDEPTH != OTHS_LIMIT && OTHL_BADDEPTH != 4 /* OTHE_NOROOM, OTHT_NOROOM */ &&
                  OTHL_BADDEPTH != OTHS_BADWINDOW,
              "a status of its own");
static_assert(OTHS_MAX_EMPTIES == oths::kMaxEmpties && OTHM_MAX_DEPTH == othm::kMaxDepth && OTH_PASS == othl::kPassMove &&
                  OTHS_NO_MOVE == othl::kNoMove && OTHS_LIMIT == oths::kLimit && OTHM_LIMIT == othm::kLimit,
              "header and core disagree");
// the longest line: a pass before every move
static_assert(2 * OTHS_MAX_EMPTIES <= OTHL_LINE_STRIDE && 2 * OTHM_MAX_DEPTH <= OTHL_LINE_STRIDE, "the row holds it");

namespace {

using othm::u32;
using othm::u64;

constexpr int kLineBlock = 64;  // one wave
using othd::DeviceRules;
using othd::kRefillMin;
using othd::status_of;
using SolveStack = othd::LdsStack7<kLineBlock>;
using SearchStack = othd::LdsStack9<kLineBlock>;
static_assert(SolveStack::kFields == oths::kFields && SearchStack::kFields == othm::kFields, "the frames' words");

// a position's row of the line: padded when the lane takes the position
struct LineRow {
    uint8_t* row;  // NULL: no line
    __device__ __forceinline__ void pad() const {
        if (!row) return;
#pragma unroll
        for (int q = 0; q < OTHL_LINE_STRIDE / 16; q++) reinterpret_cast<uint4*>(row)[q] = make_uint4(~0u, ~0u, ~0u, ~0u);
    }
    __device__ __forceinline__ void move(u32 k, u32 code) const {
        if (row && k < (u32)OTHL_LINE_STRIDE) row[k] = (uint8_t)code;
    }
    __device__ __forceinline__ void clear(u32) const { pad(); }
};

// V: int8_t (the solver) or int32_t (the search)
template <class V>
struct LineArgs {
    const u64* boards;
    const uint8_t* turn;
    const uint8_t* depths;  // the search: NULL = `depth` everywhere
    uint8_t* line;
    uint8_t* length;
    V* value;
    uint8_t* best_move;
    uint8_t* status;
    u32* nodes;
    u64* end_boards;
    uint8_t* end_turn;
    unsigned long long* work;
    u64 n;
    u64 total;  // n + lanes of the grid: what the launch's requests add up to
    u32 limit;
    int max_empties;  // the solver
    int depth;        // the search
    int8_t w[OTH_EVAL_WEIGHTS];
};

// position i's outputs: the walk W has ended; `white`: the root mover is White
template <class V>
__device__ __forceinline__ void emit(const LineArgs<V>& a, u64 i, const othl::Walk& W, bool white) {
    const bool white_to_move = white == W.root_side;
    if (a.length) a.length[i] = (uint8_t)W.len;
    if (a.value) a.value[i] = (V)W.value;
    if (a.best_move) a.best_move[i] = (uint8_t)W.move;
    if (a.status) a.status[i] = (uint8_t)W.status;
    if (a.nodes) a.nodes[i] = othl::nodes32(W);
    if (a.end_boards)
        reinterpret_cast<ulonglong2*>(a.end_boards)[i] =
            white_to_move ? make_ulonglong2(W.O, W.P) : make_ulonglong2(W.P, W.O);
    if (a.end_turn) a.end_turn[i] = white_to_move ? OTH_WHITE : OTH_BLACK;
}

__global__ __launch_bounds__(kLineBlock) void line_exact_walk(LineArgs<int8_t> a) {
    __shared__ u32 frames[oths::kFrames * oths::kFields * kLineBlock];
    const u32 lane = threadIdx.x;
    SolveStack stk{frames + lane};
    oths::Lane L;
    L.depth = -1;
    othl::Walk W;
    LineRow row{nullptr};
    bool white = false;
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
                    white = a.turn && a.turn[g] == OTH_WHITE;
                    const u32 st = oths::classify(b.x, b.y, 64 - __popcll(b.x | b.y), a.max_empties);
                    row.row = a.line ? a.line + g * OTHL_LINE_STRIDE : nullptr;
                    row.pad();
                    if (st == oths::kSolved) {
                        othl::begin_solve(W, L, white ? b.y : b.x, white ? b.x : b.y);
                        idx = g;
                    } else {
                        othl::open(W, white ? b.y : b.x, white ? b.x : b.y, 0, st);
                        emit(a, g, W, white);
                    }
                }
            }
        }
        if (L.depth >= 0) {
            oths::advance<DeviceRules>(L, stk, a.limit);
            if (L.depth < 0 && !othl::follow_solve<DeviceRules>(W, L, row)) emit(a, idx, W, white);
        }
    }
}

// the persistent loop of both search kernels; kOrdered: order_core.hpp's machine
template <bool kOrdered>
__device__ __forceinline__ void line_depth_body(const LineArgs<int32_t>& a) {
    __shared__ u32 frames[othm::kFrames * othm::kFields * kLineBlock];
    __shared__ int table[othm::kEvalTable];
    const u32 lane = threadIdx.x;
    if (lane < (u32)othm::kEvalTable) othm::widen_weight(a.w, (int)lane, table);
    __syncthreads();
    SearchStack stk{frames + lane};
    othm::Lane L;
    L.depth = -1;
    othm::Order Q;  // (unused, and gone, when !kOrdered)
    othm::order_reset(Q);
    othl::Walk W;
    LineRow row{nullptr};
    bool white = false;
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
                    white = a.turn && a.turn[g] == OTH_WHITE;
                    const u32 plies = a.depths ? (u32)a.depths[g] : (u32)a.depth;
                    const u32 st = (b.x & b.y) ? othm::kInvalid : othl::classify_depth(plies);
                    row.row = a.line ? a.line + g * OTHL_LINE_STRIDE : nullptr;
                    row.pad();
                    if (st == othm::kSearched) {
                        othl::begin_search(W, L, white ? b.y : b.x, white ? b.x : b.y, (int)plies);
                        othm::order_reset(Q);
                        idx = g;
                    } else {
                        othl::open(W, white ? b.y : b.x, white ? b.x : b.y, 0, st);
                        emit(a, g, W, white);
                    }
                }
            }
        }
        if (L.depth >= 0) {
            if constexpr (kOrdered)
                othm::advance_ordered<DeviceRules, true>(L, Q, stk, table, a.limit);
            else
                othm::advance<DeviceRules>(L, stk, table, a.limit);
            if (L.depth < 0) {
                if (othl::follow_search<DeviceRules>(W, L, row))
                    othm::order_reset(Q);
                else
                    emit(a, idx, W, white);
            }
        }
    }
}

__global__ __launch_bounds__(kLineBlock) void line_depth_walk(LineArgs<int32_t> a) { line_depth_body<false>(a); }
__global__ __launch_bounds__(kLineBlock) void line_depth_ordered_walk(LineArgs<int32_t> a) {
    line_depth_body<true>(a);
}

// one cache per kernel: the solver's, the search's, the ordered search's
othd::ResidentBlocks g_resident[3];

int solve_line_grid(int64_t n) {
    return othd::launch_grid(g_resident[0], reinterpret_cast<const void*>(line_exact_walk), kLineBlock, n,
                             "OTH_SOLVE_BLOCKS");
}

int search_line_grid(int64_t n, int order) {
    const void* kernel = order ? reinterpret_cast<const void*>(line_depth_ordered_walk)
                               : reinterpret_cast<const void*>(line_depth_walk);
    return othd::launch_grid(g_resident[1 + order], kernel, kLineBlock, n, "OTH_SEARCH_BLOCKS");
}

template <class V>
void fill(LineArgs<V>& a, const uint64_t* boards, const uint8_t* turn, uint32_t limit, uint8_t* line, uint8_t* length,
          V* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes, uint64_t* end_boards, uint8_t* end_turn,
          uint64_t* work, int64_t n, int grid) {
    a.boards = boards;
    a.turn = turn;
    a.depths = nullptr;
    a.line = line;
    a.length = length;
    a.value = value;
    a.best_move = best_move;
    a.status = status;
    a.nodes = nodes;
    a.end_boards = end_boards;
    a.end_turn = end_turn;
    a.work = reinterpret_cast<unsigned long long*>(work);
    a.n = (u64)n;
    a.total = (u64)n + (u64)grid * kLineBlock;
    a.limit = limit;
    a.max_empties = 0;
    a.depth = 0;
    for (int k = 0; k < OTH_EVAL_WEIGHTS; k++) a.w[k] = 0;
}

// the rows are padded with 16-byte stores, the end boards written as one
inline bool misaligned(const void* line, const void* end_boards) {
    return ((uintptr_t)line & 15) || ((uintptr_t)end_boards & 15);
}

}  // namespace

extern "C" {

int othl_solve_line(const uint64_t* boards, const uint8_t* turn, int max_empties, uint32_t node_limit, uint8_t* line,
                    uint8_t* length, int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
                    uint64_t* end_boards, uint8_t* end_turn, uint64_t* work, int64_t n, void* stream) {
    if (n < 0 || !work || max_empties < 0 || max_empties > OTHS_MAX_EMPTIES || (n > 0 && !boards) ||
        misaligned(line, end_boards))
        return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    const int grid = solve_line_grid(n);
    if (grid <= 0) return status_of(hipErrorInvalidDevice);
    LineArgs<int8_t> a;
    fill(a, boards, turn, node_limit ? node_limit : OTHS_DEFAULT_NODE_LIMIT, line, length, value, best_move, status,
         nodes, end_boards, end_turn, work, n, grid);
    a.max_empties = max_empties;
    line_exact_walk<<<(unsigned)grid, kLineBlock, 0, (hipStream_t)stream>>>(a);
    return status_of(hipGetLastError());
}

int othl_search_line(const uint64_t* boards, const uint8_t* turn, int depth, const uint8_t* depth_per_position,
                     int order, const int8_t* weights, uint32_t node_limit, uint8_t* line, uint8_t* length,
                     int32_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes, uint64_t* end_boards,
                     uint8_t* end_turn, uint64_t* work, int64_t n, void* stream) {
    if (order < 0 || order > OTHO_MAX_ORDER) return OTH_EINVAL;
    if (n < 0 || !work || !weights || (!depth_per_position && (depth < 1 || depth > OTHM_MAX_DEPTH)) ||
        (n > 0 && !boards) || misaligned(line, end_boards))
        return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    const int grid = search_line_grid(n, order);
    if (grid <= 0) return status_of(hipErrorInvalidDevice);
    LineArgs<int32_t> a;
    fill(a, boards, turn, node_limit ? node_limit : OTHM_DEFAULT_NODE_LIMIT, line, length, value, best_move, status,
         nodes, end_boards, end_turn, work, n, grid);
    a.depths = depth_per_position;
    a.depth = depth_per_position ? 0 : depth;
    for (int k = 0; k < OTH_EVAL_WEIGHTS; k++) a.w[k] = weights[k];
    if (order)
        line_depth_ordered_walk<<<(unsigned)grid, kLineBlock, 0, (hipStream_t)stream>>>(a);
    else
        line_depth_walk<<<(unsigned)grid, kLineBlock, 0, (hipStream_t)stream>>>(a);
    return status_of(hipGetLastError());
}

int othl_solve_line_grid(int64_t n) {
    return othd::grid_answer(n, [&] { return solve_line_grid(n); });
}

int othl_search_line_grid(int64_t n, int order) {
    if (order < 0 || order > OTHO_MAX_ORDER) return OTH_EINVAL;
    return othd::grid_answer(n, [&] { return search_line_grid(n, order); });
}

}  // extern "C"
