// moves.hip — the value of every root move, for gfx950
// (include/othello_moves.h).
//
// Each call is three steps on the caller's stream:
//   1. EXPAND: one thread per position classifies it and writes one task per
//      root move (the board after the move, the opponent to move) or one for a
//      forced pass (the same board, the opponent to move) into scratch;
//   2. the tasks are solved by the launch code that exists (oths_solve,
//      othe_solve, othh_solve_hashed, called through their C-ABI: the old
//      kernels are reused untouched) or searched by search_moves_kernel below;
//   3. FINISH: one wave per position, lane s owning square s, scatters minus
//      the tasks' values into the row and reduces value, move, status, nodes.
//
// The exact calls give every position max(max_empties, 1) task slots, so the
// task count is known on the host without a count or a synchronisation; unused
// slots hold the empty board (64 empties: SKIPPED at once).
//
// The search cannot reuse othm_search (its leaves are scored from the side of
// ITS root mover), so it has a kernel of its own and is free to pack: the
// expand kernel reserves each position's tasks in one list with an atomic on
// a counter in scratch, and search_moves_kernel — search.hip's persistent
// one-wave loop, same frames, same table, same refill at kRefillMin idle lanes
// — claims indices of that list.  Claiming (position, square) pairs directly
// would spend a refill request on every non-move square (about six in seven)
// and a moves() per claim; the list costs 26 B of scratch per task.
#include "../../include/othello_moves.h"
#include "../../include/othello_search.h"
#include "../../include/othello_solve.h"
#include "../../include/othello_solve_hash.h"
#include "../../include/othello_solve_tree.h"
#include "device_common.hpp"
#include "search_core.hpp"
#include "solve_core.hpp"

static_assert(OTHA_SEARCH_SLOTS == 64, "a task per square at most");

namespace {

using othd::DeviceRules;
using othd::kRefillMin;
using othd::status_of;
using othd::u32;
using othd::u64;

constexpr int kBlock = 256;       // expand: a thread per position; finish: a wave per position
constexpr int kSearchBlock = 64;  // one wave, as search.hip
using LdsStack = othd::LdsStack9<kSearchBlock>;

// what the expand kernel found at a root
constexpr uint8_t kKindMoves = 0, kKindPass = 1, kKindOver = 2, kKindInvalid = 3, kKindSkipped = 4;
constexpr uint8_t kNoSquare = 255;
constexpr u32 kDone = 1;  // OTHS_SOLVED == OTHM_SEARCHED
static_assert(OTHS_SOLVED == kDone && OTHM_SEARCHED == kDone && OTHS_INVALID == OTHM_INVALID &&
                  OTHS_LIMIT == OTHM_LIMIT && OTHS_NO_MOVE == OTHM_NO_MOVE,
              "the solver's and the search's statuses are one set here");

inline int64_t round8(int64_t x) { return (x + 7) & ~(int64_t)7; }

// ---- the exact calls' scratch: K slots per position, N = n * K tasks ----
struct SolveScratch {
    u64* boards;      // [N][2] black, white
    u32* nodes;       // [N]
    int8_t* value;    // [N]
    uint8_t* status;  // [N]
    uint8_t* turn;    // [N]
    uint8_t* sq;      // [N] the root move, 64 for the pass task, 255 for an unused slot
    uint8_t* kind;    // [n]
    uint8_t* count;   // [n] tasks of the position
    char* rest;       // the split solver's own scratch
    int64_t bytes;    // up to `rest`
};

SolveScratch solve_scratch(void* base, int64_t n, int64_t N) {
    SolveScratch s;
    char* p = static_cast<char*>(base);
    s.boards = reinterpret_cast<u64*>(p);
    s.nodes = reinterpret_cast<u32*>(p + 16 * N);
    s.value = reinterpret_cast<int8_t*>(p + 20 * N);
    s.status = reinterpret_cast<uint8_t*>(p + 21 * N);
    s.turn = reinterpret_cast<uint8_t*>(p + 22 * N);
    s.sq = reinterpret_cast<uint8_t*>(p + 23 * N);
    s.kind = reinterpret_cast<uint8_t*>(p + 24 * N);
    s.count = s.kind + n;
    s.bytes = round8(24 * N + 2 * n);
    s.rest = p + s.bytes;
    return s;
}

// ---- the search's scratch: one packed list of at most cap = n * 64 tasks ----
struct SearchScratch {
    unsigned long long* total;  // tasks in the list
    u64* first;                 // [n] the position's first task
    u64* boards;                // [cap][2] the task's mover's discs, the other side's (the root mover's)
    int32_t* value;             // [cap]
    u32* nodes;                 // [cap]
    uint8_t* status;            // [cap]
    uint8_t* sq;                // [cap]
    uint8_t* kind;              // [n]
    uint8_t* count;             // [n]
    int64_t bytes;
};

SearchScratch search_scratch(void* base, int64_t n) {
    const int64_t cap = n * OTHA_SEARCH_SLOTS;
    SearchScratch s;
    char* p = static_cast<char*>(base);
    s.total = reinterpret_cast<unsigned long long*>(p);
    s.boards = reinterpret_cast<u64*>(p + 16);  // (16-byte rows: read as one ulonglong2)
    s.first = reinterpret_cast<u64*>(p + 16 + 16 * cap);
    char* q = p + 16 + 16 * cap + 8 * n;
    s.value = reinterpret_cast<int32_t*>(q);
    s.nodes = reinterpret_cast<u32*>(q + 4 * cap);
    s.status = reinterpret_cast<uint8_t*>(q + 8 * cap);
    s.sq = reinterpret_cast<uint8_t*>(q + 9 * cap);
    s.kind = reinterpret_cast<uint8_t*>(q + 10 * cap);
    s.count = s.kind + n;
    s.bytes = round8(16 + 8 * n + 26 * cap + 2 * n);
    return s;
}

// ---- expand ----

struct ExpandSolveArgs {
    const u64* boards;
    const uint8_t* turn;
    u64* cboards;
    uint8_t* cturn;
    uint8_t* csq;
    uint8_t* kind;
    uint8_t* count;
    u64 n;
    int max_empties;
    int slots;  // max(max_empties, 1)
};

__global__ __launch_bounds__(kBlock) void moves_expand_solve(ExpandSolveArgs a) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.boards)[i];
    const bool white = a.turn && a.turn[i] == OTH_WHITE;
    const u32 st = oths::classify(b.x, b.y, 64 - __popcll(b.x | b.y), a.max_empties);
    const u64 P = white ? b.y : b.x, O = white ? b.x : b.y;
    u64 M = 0;
    uint8_t kind = st == oths::kInvalid ? kKindInvalid : kKindSkipped;
    bool pass = false;
    if (st == oths::kSolved) {
        M = DeviceRules::moves(P, O);
        pass = M == 0 && DeviceRules::moves(O, P) != 0;
        kind = M ? kKindMoves : pass ? kKindPass : kKindOver;
    }
    a.kind[i] = kind;
    a.count[i] = (uint8_t)(pass ? 1 : __popcll(M));  // (a solved position has at most `slots` moves)
    const uint8_t other = white ? OTH_BLACK : OTH_WHITE;
    const u64 t0 = i * (u64)a.slots;
    for (int j = 0; j < a.slots; j++) {
        u64 X = 0, Y = 0;  // the task's mover's discs, the root mover's
        uint8_t sq = kNoSquare;
        if (M) {
            sq = (uint8_t)DeviceRules::lowest(M);
            M &= M - 1;
            const u64 f = DeviceRules::flips(sq, P, O);
            X = O & ~f;
            Y = P | f | (1ull << sq);
        } else if (pass && j == 0) {
            sq = OTH_PASS;
            X = O;
            Y = P;
        }
        // the opponent is to move: White's discs are X when the root mover is Black
        reinterpret_cast<ulonglong2*>(a.cboards)[t0 + j] = white ? make_ulonglong2(X, Y) : make_ulonglong2(Y, X);
        a.cturn[t0 + j] = other;
        a.csq[t0 + j] = sq;
    }
}

struct ExpandSearchArgs {
    const u64* boards;
    const uint8_t* turn;
    unsigned long long* total;
    u64* first;
    u64* tboards;
    uint8_t* tsq;
    uint8_t* kind;
    uint8_t* count;
    u64 n;
};

__global__ __launch_bounds__(kBlock) void moves_expand_search(ExpandSearchArgs a) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.boards)[i];
    const bool white = a.turn && a.turn[i] == OTH_WHITE;
    const u64 P = white ? b.y : b.x, O = white ? b.x : b.y;
    u64 M = 0;
    bool pass = false;
    uint8_t kind = kKindInvalid;
    if ((b.x & b.y) == 0) {
        M = DeviceRules::moves(P, O);
        pass = M == 0 && DeviceRules::moves(O, P) != 0;
        kind = M ? kKindMoves : pass ? kKindPass : kKindOver;
    }
    const u32 c = pass ? 1u : (u32)__popcll(M);  // <= 60 < OTHA_SEARCH_SLOTS
    u64 t = 0;
    if (c) t = atomicAdd(a.total, (unsigned long long)c);
    a.kind[i] = kind;
    a.count[i] = (uint8_t)c;
    a.first[i] = t;
    if (pass) {
        reinterpret_cast<ulonglong2*>(a.tboards)[t] = make_ulonglong2(O, P);
        a.tsq[t] = OTH_PASS;
    }
    for (; M; M &= M - 1, t++) {
        const u32 sq = DeviceRules::lowest(M);
        const u64 f = DeviceRules::flips(sq, P, O);
        reinterpret_cast<ulonglong2*>(a.tboards)[t] = make_ulonglong2(O & ~f, P | f | (1ull << sq));
        a.tsq[t] = (uint8_t)sq;
    }
}

// ---- the search over tasks ----

struct SearchMovesArgs {
    const unsigned long long* total;  // tasks in the list (written by the expand kernel)
    const u64* tboards;
    const uint8_t* tsq;
    int32_t* tvalue;
    uint8_t* tstatus;
    u32* tnodes;
    unsigned long long* work;
    u32 limit;
    int depth;
    int8_t w[OTH_EVAL_WEIGHTS];
};

__device__ __forceinline__ void emit_task(const SearchMovesArgs& a, u64 t, int value, u32 status, u32 nodes) {
    a.tvalue[t] = value;
    a.tstatus[t] = (uint8_t)status;
    a.tnodes[t] = nodes;
}

// search.hip's persistent loop over the task list.  A task's value is
// S(task, its mover, rem) from ITS mover's side with the leaves scored from the
// other side's, the root mover's: start_child() clears the root-side flag.
__global__ __launch_bounds__(kSearchBlock) void search_moves_kernel(SearchMovesArgs a) {
    __shared__ u32 frames[othm::kFrames * othm::kFields * kSearchBlock];
    __shared__ int table[othm::kEvalTable];
    const u32 lane = threadIdx.x;
    if (lane < (u32)othm::kEvalTable) othm::widen_weight(a.w, (int)lane, table);
    __syncthreads();
    const u64 n = *a.total;
    const u64 total = n + (u64)gridDim.x * kSearchBlock;  // what the launch's requests add up to
    LdsStack stk{frames + lane};
    othm::Lane L;
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
        if (wantm != 0 && ((int)cnt >= kRefillMin || busym == 0)) {
            const u64 g = othd::take(a.work, total, wantm, cnt, lane);
            if (want) {
                if (g >= n) {
                    exhausted = true;
                } else {
                    const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.tboards)[g];  // x to move
                    const bool pass = a.tsq[g] == OTH_PASS;
                    const u64 cm = DeviceRules::moves(b.x, b.y);
                    if (!pass && a.depth == 1) {
                        // a leaf, scored where it is made (search_core.hpp's rule
                        // with the root side having just moved: it owns b.y)
                        const u64 om = DeviceRules::moves(b.y, b.x);
                        const int score = (cm | om) == 0
                                              ? othm::kTerminal * (__popcll(b.y) - __popcll(b.x))
                                              : othm::eval<DeviceRules>(table, b.y, om, (u32)__popcll(b.x | b.y));
                        emit_task(a, g, -score, othm::kSearched, 0u);
                    } else {
                        othm::start_child(L, b.x, b.y, cm, pass ? a.depth : a.depth - 1);
                        idx = g;
                    }
                }
            }
        }
        if (L.depth >= 0) {
            othm::advance<DeviceRules>(L, stk, table, a.limit);
            if (L.depth < 0) emit_task(a, idx, L.value, L.status, L.nodes);
        }
    }
}

// ---- finish ----

template <class V>
struct FinishArgs {
    const u64* boards;
    const uint8_t* turn;
    const V* tvalue;
    const uint8_t* tstatus;
    const u32* tnodes;
    const uint8_t* tsq;
    const uint8_t* kind;
    const uint8_t* count;
    const u64* first;  // NULL: position i's tasks start at i * slots
    int slots;
    V* move_value;
    V* value;
    uint8_t* best_move;
    uint8_t* status;
    u32* nodes;
    u64 n;
    int scale;  // of a finished game's disc difference
    V not_a_move, unknown;
};

// a wave per position: lane s owns square s; every lane walks the position's
// tasks (uniform loads) and lane 0 writes the position's answers
template <class V>
__global__ __launch_bounds__(kBlock) void moves_finish(FinishArgs<V> a) {
    const u64 i = (u64)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
    if (i >= a.n) return;
    const u32 s = threadIdx.x & 63u;
    const u32 kind = a.kind[i];
    const u32 c = a.count[i];
    const u64 t0 = a.first ? a.first[i] : i * (u64)a.slots;
    V row = a.not_a_move;
    int best = INT32_MIN;
    u32 mv = OTHS_NO_MOVE, st = kDone;
    u64 nodes = c;
    bool unknown = false;
    for (u32 j = 0; j < c; j++) {
        const u32 sq = a.tsq[t0 + j], ts = a.tstatus[t0 + j];
        const int v = -(int)a.tvalue[t0 + j];
        nodes += a.tnodes[t0 + j];
        st = ts > st ? ts : st;
        if (ts != kDone) {
            unknown = true;
            if (sq == s) row = a.unknown;
        } else {
            if (sq == s) row = (V)v;
            if (v > best) {  // (the tasks are in square order: strict keeps the lowest)
                best = v;
                mv = sq;
            }
        }
    }
    if (a.move_value) a.move_value[i * 64 + s] = row;
    if (s != 0) return;
    int value = best;
    if (kind == kKindOver) {
        const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.boards)[i];
        const int d = __popcll(b.x) - __popcll(b.y);
        value = a.scale * ((a.turn && a.turn[i] == OTH_WHITE) ? -d : d);
    } else if (kind == kKindInvalid || kind == kKindSkipped) {
        value = 0;
        st = kind == kKindInvalid ? OTHS_INVALID : OTHS_SKIPPED;
    } else if (unknown) {
        value = 0;
        mv = OTHS_NO_MOVE;
    }
    if (a.value) a.value[i] = (V)value;
    if (a.best_move) a.best_move[i] = (uint8_t)mv;
    if (a.status) a.status[i] = (uint8_t)st;
    if (a.nodes) a.nodes[i] = nodes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)nodes;
}

constexpr int64_t kMaxTasks = (int64_t)1 << 55;

int64_t slots_of(int max_empties) { return max_empties > 1 ? max_empties : 1; }

unsigned blocks_for(int64_t items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

// steps 1 and 3 of the exact calls around `solve_tasks`, which launches step 2
template <class F>
int solve_moves(const uint64_t* boards, const uint8_t* turn, int max_empties, int8_t* move_value, int8_t* value,
                uint8_t* best_move, uint8_t* status, uint32_t* nodes, const SolveScratch& s, int64_t n,
                hipStream_t stream, F solve_tasks) {
    const int slots = (int)slots_of(max_empties);
    ExpandSolveArgs e;
    e.boards = boards;
    e.turn = turn;
    e.cboards = s.boards;
    e.cturn = s.turn;
    e.csq = s.sq;
    e.kind = s.kind;
    e.count = s.count;
    e.n = (u64)n;
    e.max_empties = max_empties;
    e.slots = slots;
    moves_expand_solve<<<blocks_for(n, kBlock), kBlock, 0, stream>>>(e);
    int rc = status_of(hipGetLastError());
    if (rc != OTH_OK) return rc;
    rc = solve_tasks();
    if (rc != OTH_OK) return rc;
    FinishArgs<int8_t> f;
    f.boards = boards;
    f.turn = turn;
    f.tvalue = s.value;
    f.tstatus = s.status;
    f.tnodes = s.nodes;
    f.tsq = s.sq;
    f.kind = s.kind;
    f.count = s.count;
    f.first = nullptr;
    f.slots = slots;
    f.move_value = move_value;
    f.value = value;
    f.best_move = best_move;
    f.status = status;
    f.nodes = nodes;
    f.n = (u64)n;
    f.scale = 1;
    f.not_a_move = OTHA_NOT_A_MOVE;
    f.unknown = OTHA_UNKNOWN;
    moves_finish<int8_t><<<blocks_for(n, kBlock / 64), kBlock, 0, stream>>>(f);
    return status_of(hipGetLastError());
}

othd::ResidentBlocks g_resident;  // search_moves_kernel's

}  // namespace

extern "C" {

int64_t otha_solve_moves_scratch_bytes(int64_t n, int max_empties) {
    if (n < 0 || max_empties < 0 || max_empties > OTHS_MAX_EMPTIES || n > kMaxTasks / 16) return OTH_EINVAL;
    return solve_scratch(nullptr, n, n * slots_of(max_empties)).bytes;
}

int otha_solve_moves(const uint64_t* boards, const uint8_t* turn, int max_empties, uint32_t node_limit,
                     int8_t* move_value, int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
                     void* scratch, int64_t scratch_bytes, uint64_t* work, int64_t n, void* stream) {
    const int64_t need = otha_solve_moves_scratch_bytes(n, max_empties);
    if (need < 0 || !work || (n > 0 && (!boards || !scratch || ((uintptr_t)scratch & 15) || scratch_bytes < need)))
        return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    const int64_t N = n * slots_of(max_empties);
    const SolveScratch s = solve_scratch(scratch, n, N);
    return solve_moves(boards, turn, max_empties, move_value, value, best_move, status, nodes, s, n,
                       (hipStream_t)stream, [&] {
                           return oths_solve(s.boards, s.turn, max_empties, node_limit, s.value, nullptr, s.status,
                                             s.nodes, work, N, stream);
                       });
}

int64_t otha_solve_moves_split_scratch_bytes(int64_t n, int max_empties, int32_t nodes_per_position) {
    if (n < 0 || max_empties < 0 || max_empties > OTHE_MAX_EMPTIES || n > kMaxTasks / 16) return OTH_EINVAL;
    const int64_t N = n * slots_of(max_empties);
    const int64_t inner = othe_scratch_bytes(N, nodes_per_position);
    if (inner < 0) return OTH_EINVAL;
    return solve_scratch(nullptr, n, N).bytes + inner;
}

int otha_solve_moves_split(const uint64_t* boards, const uint8_t* turn, int max_empties, int task_empties, int order,
                           uint32_t node_limit, int32_t nodes_per_position, int hash_bits, int hash_min_empties,
                           void* table, int64_t table_bytes, int8_t* move_value, int8_t* value, uint8_t* best_move,
                           uint8_t* status, uint32_t* nodes, void* scratch, int64_t scratch_bytes, uint64_t* work,
                           int64_t n, void* stream) {
    if (table) {  // othh_solve_hashed's checks, made before anything is launched
        const int64_t tb = othh_hash_bytes(hash_bits);
        if (tb < 0 || table_bytes < tb || ((uintptr_t)table & (OTHH_ENTRY_BYTES - 1)) ||
            hash_min_empties < OTHH_MIN_EMPTIES_LO || hash_min_empties > OTHH_MIN_EMPTIES_HI)
            return OTH_EINVAL;
    }
    if (task_empties < 1 || task_empties > OTHS_MAX_EMPTIES || order < 0 || order > 1) return OTH_EINVAL;
    const int64_t need = otha_solve_moves_split_scratch_bytes(n, max_empties, nodes_per_position);
    if (need < 0 || !work || (n > 0 && (!boards || !scratch || ((uintptr_t)scratch & 15) || scratch_bytes < need)))
        return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    const int64_t N = n * slots_of(max_empties);
    const SolveScratch s = solve_scratch(scratch, n, N);
    const int64_t inner = need - s.bytes;
    return solve_moves(boards, turn, max_empties, move_value, value, best_move, status, nodes, s, n,
                       (hipStream_t)stream, [&] {
                           if (table)
                               return othh_solve_hashed(s.boards, s.turn, max_empties, task_empties, order, node_limit,
                                                        s.value, nullptr, s.status, s.nodes, s.rest, inner,
                                                        nodes_per_position, work, N, hash_bits, hash_min_empties,
                                                        table, table_bytes, stream);
                           return othe_solve(s.boards, s.turn, max_empties, task_empties, order, node_limit, s.value,
                                             nullptr, s.status, s.nodes, s.rest, inner, nodes_per_position, work, N,
                                             stream);
                       });
}

int64_t otha_search_moves_scratch_bytes(int64_t n) {
    if (n < 0 || n > kMaxTasks / OTHA_SEARCH_SLOTS) return OTH_EINVAL;
    return search_scratch(nullptr, n).bytes;
}

int otha_search_moves(const uint64_t* boards, const uint8_t* turn, int depth, const int8_t* weights,
                      uint32_t node_limit, int32_t* move_value, int32_t* value, uint8_t* best_move, uint8_t* status,
                      uint32_t* nodes, void* scratch, int64_t scratch_bytes, uint64_t* work, int64_t n, void* stream) {
    const int64_t need = otha_search_moves_scratch_bytes(n);
    if (need < 0 || !work || !weights || depth < 1 || depth > OTHM_MAX_DEPTH ||
        (n > 0 && (!boards || !scratch || ((uintptr_t)scratch & 15) || scratch_bytes < need)))
        return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    // the task count is the device's: a wave per 8 positions' worth of lanes
    // (about 8 moves each), capped like othm_search's grid
    static_assert(kSearchBlock % 8 == 0, "a block per 8 positions");
    const int grid = othd::launch_grid(g_resident, reinterpret_cast<const void*>(search_moves_kernel), kSearchBlock,
                                       n * (kSearchBlock / 8), "OTH_SEARCH_BLOCKS");
    if (grid <= 0) return status_of(hipErrorInvalidDevice);
    const SearchScratch s = search_scratch(scratch, n);
    hipStream_t q = (hipStream_t)stream;
    int rc = status_of(hipMemsetAsync(s.total, 0, sizeof(*s.total), q));
    if (rc != OTH_OK) return rc;
    ExpandSearchArgs e;
    e.boards = boards;
    e.turn = turn;
    e.total = s.total;
    e.first = s.first;
    e.tboards = s.boards;
    e.tsq = s.sq;
    e.kind = s.kind;
    e.count = s.count;
    e.n = (u64)n;
    moves_expand_search<<<blocks_for(n, kBlock), kBlock, 0, q>>>(e);
    rc = status_of(hipGetLastError());
    if (rc != OTH_OK) return rc;
    SearchMovesArgs a;
    a.total = s.total;
    a.tboards = s.boards;
    a.tsq = s.sq;
    a.tvalue = s.value;
    a.tstatus = s.status;
    a.tnodes = s.nodes;
    a.work = reinterpret_cast<unsigned long long*>(work);
    a.limit = node_limit ? node_limit : OTHM_DEFAULT_NODE_LIMIT;
    a.depth = depth;
    for (int k = 0; k < OTH_EVAL_WEIGHTS; k++) a.w[k] = weights[k];
    search_moves_kernel<<<(unsigned)grid, kSearchBlock, 0, q>>>(a);
    rc = status_of(hipGetLastError());
    if (rc != OTH_OK) return rc;
    FinishArgs<int32_t> f;
    f.boards = boards;
    f.turn = turn;
    f.tvalue = s.value;
    f.tstatus = s.status;
    f.tnodes = s.nodes;
    f.tsq = s.sq;
    f.kind = s.kind;
    f.count = s.count;
    f.first = s.first;
    f.slots = 0;
    f.move_value = move_value;
    f.value = value;
    f.best_move = best_move;
    f.status = status;
    f.nodes = nodes;
    f.n = (u64)n;
    f.scale = OTHM_TERMINAL_SCALE;
    f.not_a_move = OTHA_NOT_A_MOVE32;
    f.unknown = OTHA_UNKNOWN32;
    moves_finish<int32_t><<<blocks_for(n, kBlock / 64), kBlock, 0, q>>>(f);
    return status_of(hipGetLastError());
}

}  // extern "C"
