// perft.hip — perft, the number of move paths of a batch of positions, for
// gfx950 (include/othello_perft.h).
//
// Each call is, on the caller's stream:
//   1. memset nodes: the level counters and flags and the positions' limit
//      flags in scratch, and the outputs the count kernel adds into;
//   2. LEVEL 0: one thread per position writes one task per valid position;
//   3. EXPAND, `split` times: a fixed grid walks the previous level's list (its
//      length is read on the device) and replaces every task by its children,
//      moves.hip's expand with a list for input.  A wave reserves the room of
//      its 64 tasks' children with one atomic (a scan of the counts); a
//      reservation that ends beyond the list makes the level VOID;
//   4. COUNT: search.hip's persistent one-wave loop over the tasks of the last
//      level that is not void, perft_core.hpp's machine in every lane, frames
//      in LDS indexed [depth][field][lane];
//   5. FINISH: a wave per position writes status and clears the counts of a
//      position one of whose tasks met the limit.
// Nothing is read on the host between the steps.
//
// The count kernel's adds.  A finished task's count belongs to leaves[i] and
// to its root move's column of the row.  The tasks of ONE position (a million
// of them at split 8) would make as many atomics on one address, some 10 ns
// each (measured: 4 ms of a 5.5 ms depth-12 call).  So a lane
// keeps the sum of consecutive tasks with the same (position, root square),
// and when a lane's key changes, and when the wave runs out of tasks, the WAVE
// adds (wave_flush): lanes with one key are summed across the wave and make
// one atomic.  With one position a wave makes a handful of adds in all, with a
// batch at split 0 one per task as the header says.  Integer sums commute: the
// outputs do not depend on it.
#include "../../include/othello_perft.h"
#include "device_common.hpp"
#include "perft_core.hpp"

static_assert(OTHC_MAX_DEPTH == othc::kMaxDepth && OTHC_COUNTED == othc::kCounted && OTHC_INVALID == othc::kInvalid &&
                  OTHC_LIMIT == othc::kLimit && OTHC_BADDEPTH == othc::kBadDepth,
              "the header's constants are the core's");
static_assert(OTHC_MAX_TASKS == (1 << othc::kSqShift), "a position index fits the task word");
static_assert(OTH_PASS == othc::kSqPass, "a root pass is tagged OTH_PASS");
static_assert(OTHC_MAX_DEPTH <= 15, "plies left fit the task word's four bits");

namespace {

using othd::DeviceRules;
using othd::kRefillMin;
using othd::status_of;
using othd::u32;
using othd::u64;

constexpr int kBlock = 256;      // level 0: a thread per position; expand: a thread per task; finish: a wave per position
constexpr int kCountBlock = 64;  // one wave, as search.hip
constexpr int kLevels = OTHC_MAX_SPLIT + 1;

// perft_core.hpp's frames in a block of kB lanes (device_common.hpp's layout
// with six words); `base` already points at the lane's column
template <int kB>
struct LdsStack6 {
    static constexpr int kFields = 6;
    u32* base;
    __device__ __forceinline__ u32* at(int depth) const { return base + depth * (kFields * kB); }
    __device__ __forceinline__ void store(int depth, u64 P, u64 O, u64 M) {
        u32* f = at(depth);
        f[0 * kB] = (u32)P;
        f[1 * kB] = (u32)(P >> 32);
        f[2 * kB] = (u32)O;
        f[3 * kB] = (u32)(O >> 32);
        f[4 * kB] = (u32)M;
        f[5 * kB] = (u32)(M >> 32);
    }
    __device__ __forceinline__ void load(int depth, u64& P, u64& O, u64& M) const {
        const u32* f = at(depth);
        P = (u64)f[0 * kB] | ((u64)f[1 * kB] << 32);
        O = (u64)f[2 * kB] | ((u64)f[3 * kB] << 32);
        M = (u64)f[4 * kB] | ((u64)f[5 * kB] << 32);
    }
};
using LdsStack = LdsStack6<kCountBlock>;
static_assert(othc::kFrames * othc::kFields * kCountBlock * 4 == OTHC_COUNT_LDS_BYTES, "the header's LDS figure");
static_assert(othc::kFields == LdsStack::kFields, "the core's frame");

// ---- scratch ----
// [0, kHeadBytes): the levels' task counts and void flags; then the positions'
// limit flags — one memset clears both — then the two lists
constexpr int64_t kHeadBytes = 128;
static_assert(kLevels * 8 + kLevels * 4 <= kHeadBytes, "counters and flags fit the head");
constexpr int64_t kTaskBytes = 24;  // a board pair and a word

struct Scratch {
    unsigned long long* count;  // [kLevels] tasks of level k
    u32* voidf;                 // [kLevels] level k did not fit
    u32* limitf;                // [n] a task of the position met the limit
    ulonglong2* pos[2];         // [cap] the task's mover's discs, the other side's
    u64* word[2];               // [cap] perft_core.hpp's task word
    int64_t clear_bytes;        // what the memset covers
    int64_t cap;
};

inline int64_t round16(int64_t x) { return (x + 15) & ~(int64_t)15; }
inline int64_t flags_bytes(int64_t n) { return kHeadBytes + round16(4 * n); }

Scratch scratch_of(void* base, int64_t n, int64_t cap) {
    Scratch s;
    char* p = static_cast<char*>(base);
    s.count = reinterpret_cast<unsigned long long*>(p);
    s.voidf = reinterpret_cast<u32*>(p + kLevels * 8);
    s.limitf = reinterpret_cast<u32*>(p + kHeadBytes);
    s.clear_bytes = flags_bytes(n);
    char* q = p + s.clear_bytes;
    s.pos[0] = reinterpret_cast<ulonglong2*>(q);
    s.pos[1] = reinterpret_cast<ulonglong2*>(q + 16 * cap);
    s.word[0] = reinterpret_cast<u64*>(q + 32 * cap);
    s.word[1] = reinterpret_cast<u64*>(q + 40 * cap);
    s.cap = cap;
    return s;
}

// ---- level 0 ----

struct RootArgs {
    const u64* boards;
    const uint8_t* turn;
    const uint8_t* depths;
    unsigned long long* count;  // level 0's
    ulonglong2* pos;
    u64* word;
    u64 n;
    int depth;
};

__global__ __launch_bounds__(kBlock) void perft_roots(RootArgs a) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u32 lane = threadIdx.x & 63u;
    bool valid = false;
    u64 P = 0, O = 0;
    u32 rem = 0;
    if (i < a.n) {
        const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.boards)[i];
        const bool white = a.turn && a.turn[i] == OTH_WHITE;
        P = white ? b.y : b.x;
        O = white ? b.x : b.y;
        rem = a.depths ? a.depths[i] : (u32)a.depth;
        valid = (b.x & b.y) == 0 && rem <= (u32)OTHC_MAX_DEPTH;
    }
    // one add per wave (every lane of the wave is here)
    const u64 m = __ballot(valid);
    if (m == 0) return;
    u64 base = 0;
    if (lane == 0) base = atomicAdd(a.count, (unsigned long long)__popcll(m));
    base = __shfl(base, 0);
    if (!valid) return;
    const u64 t = base + (u64)__popcll(m & ((1ull << lane) - 1ull));  // < n <= cap
    a.pos[t] = make_ulonglong2(P, O);
    a.word[t] = othc::task_word(i, othc::kSqNone, rem, false);
}

// ---- expand ----

struct ExpandArgs {
    const unsigned long long* src_count;
    unsigned long long* dst_count;
    const u32* src_void;  // NULL at the first level (level 0 always fits)
    u32* dst_void;
    const ulonglong2* src_pos;
    const u64* src_word;
    ulonglong2* dst_pos;
    u64* dst_word;
    u64 cap;
};

__global__ __launch_bounds__(kBlock) void perft_expand(ExpandArgs a) {
    if (a.src_void && *a.src_void) {  // the level before is void: so is this one, the list in force stays
        if (blockIdx.x == 0 && threadIdx.x == 0) *a.dst_void = 1u;
        return;
    }
    const u64 n = *a.src_count;  // <= cap: the level before fitted
    const u32 lane = threadIdx.x & 63u;
    const u64 wave = ((u64)blockIdx.x * kBlock + threadIdx.x) >> 6, waves = ((u64)gridDim.x * kBlock) >> 6;
    for (u64 t0 = wave * 64; t0 < n; t0 += waves * 64) {  // (uniform in the wave)
        const u64 t = t0 + lane;
        u64 P = 0, O = 0, M = 0, w = 0;
        u32 c = 0;
        bool same = false, pass = false;
        if (t < n) {
            const ulonglong2 b = a.src_pos[t];
            P = b.x;
            O = b.y;
            w = a.src_word[t];
            c = 1;
            same = othc::task_final(w);
            if (!same) {
                M = DeviceRules::moves(P, O);
                if (M)
                    c = (u32)__popcll(M);
                else
                    pass = DeviceRules::moves(O, P) != 0;
            }
        }
        // the wave's reservation: an inclusive scan of c, one add by the last lane
        u32 incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 up = __shfl_up(incl, d);
            if (lane >= (u32)d) incl += up;
        }
        const u32 total = __shfl(incl, 63);
        u64 base = 0;
        if (lane == 63 && total) base = atomicAdd(a.dst_count, (unsigned long long)total);
        base = __shfl(base, 63);
        if (c == 0) continue;
        u64 d = base + incl - c;
        if (d + c > a.cap) {  // no room: the level is void, nothing of it is read
            atomicExch(a.dst_void, 1u);
            continue;
        }
        const u64 index = othc::task_index(w);
        const u32 sq0 = othc::task_sq(w), rem = othc::task_rem(w);
        if (same) {
            a.dst_pos[d] = make_ulonglong2(P, O);
            a.dst_word[d] = w;
        } else if (M == 0) {
            // a pass is a ply: the other side to move with one ply fewer; or the game is over
            a.dst_pos[d] = pass ? make_ulonglong2(O, P) : make_ulonglong2(P, O);
            a.dst_word[d] = pass ? othc::task_word(index, sq0 == othc::kSqNone ? othc::kSqPass : sq0, rem - 1, false)
                                 : othc::task_word(index, sq0, rem, true);
        } else {
            for (; M; M &= M - 1, d++) {
                const u32 sq = DeviceRules::lowest(M);
                const u64 f = DeviceRules::flips(sq, P, O);
                a.dst_pos[d] = make_ulonglong2(O & ~f, P | f | (1ull << sq));
                a.dst_word[d] = othc::task_word(index, sq0 == othc::kSqNone ? sq : sq0, rem - 1, false);
            }
        }
    }
}

// ---- count ----

struct CountArgs {
    const unsigned long long* count;  // [kLevels]
    const u32* voidf;                 // [kLevels]
    const ulonglong2* pos[2];
    const u64* word[2];
    unsigned long long* leaves;  // may be NULL
    unsigned long long* divide;  // may be NULL
    unsigned long long* nodes;   // may be NULL
    u32* limitf;
    unsigned long long* work;
    u32 limit;
    int levels;  // expand kernels launched
};

// a lane's pending sum: the counts of consecutive tasks with one (position, root square)
struct Pending {
    u64 key;  // the task word's index and square bits; kNoKey: nothing pending
    u64 leaves, nodes;
};
constexpr u64 kKeyMask = (1ull << othc::kRemShift) - 1;
constexpr u64 kNoKey = ~0ull;

__device__ __forceinline__ u64 wave_sum(u64 x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += (u64)__shfl_xor((unsigned long long)x, d);
    return x;
}

// The wave adds the pending sums of its lanes in `sel` and forgets them: the
// lanes that share a key are summed first and one of them makes the adds, so a
// wave whose lanes work below one root move makes one atomic, not 64.  Every
// lane of the wave calls it.
__device__ __forceinline__ void wave_flush(const CountArgs& a, Pending& p, bool sel, u32 lane) {
    u64 m = __ballot(sel);
    while (m) {  // (uniform: one turn per key among the selected lanes)
        const int leader = (int)__builtin_ctzll(m);
        const u64 key = (u64)__shfl((unsigned long long)p.key, leader);
        const bool mine = sel && p.key == key;
        const u64 leaves = wave_sum(mine ? p.leaves : 0ull), nodes = wave_sum(mine ? p.nodes : 0ull);
        if (lane == (u32)leader) {
            const u64 i = othc::task_index(key);
            const u32 sq = othc::task_sq(key);
            if (a.leaves && leaves) atomicAdd(a.leaves + i, (unsigned long long)leaves);
            if (a.divide && sq < 64 && leaves) atomicAdd(a.divide + i * 64 + sq, (unsigned long long)leaves);
            if (a.nodes && nodes) atomicAdd(a.nodes + i, (unsigned long long)nodes);
        }
        m &= ~__ballot(mine);
    }
    if (sel) p.key = kNoKey;
}

__global__ __launch_bounds__(kCountBlock) void perft_count_kernel(CountArgs a) {
    __shared__ u32 frames[othc::kFrames * othc::kFields * kCountBlock];
    const u32 lane = threadIdx.x;
    int lv = 0;  // the last level that is not void
    for (int k = 1; k <= a.levels; k++) {
        if (a.voidf[k]) break;
        lv = k;
    }
    const u64 n = a.count[lv];
    const ulonglong2* tpos = a.pos[lv & 1];
    const u64* tword = a.word[lv & 1];
    const u64 total = n + (u64)gridDim.x * kCountBlock;  // what the launch's requests add up to
    LdsStack stk{frames + lane};
    othc::Lane L;
    L.depth = -1;
    Pending pend{kNoKey, 0, 0};
    u64 cur = 0;
    bool exhausted = false;  // the lane has made its failing request
    for (;;) {
        const bool idle = L.depth < 0;
        const bool want = idle && !exhausted;
        const u64 wantm = __ballot(want);
        const u64 busym = __ballot(!idle);
        if ((wantm | busym) == 0) break;
        const u64 cnt = (u64)__popcll(wantm);
        bool done = false;  // the lane finished task `cur` in this turn: `count` paths, `visited` nodes
        u64 count = 1;
        u32 visited = 0;
        if (wantm != 0 && ((int)cnt >= kRefillMin || busym == 0)) {
            const u64 g = othd::take(a.work, total, wantm, cnt, lane);
            if (want) {
                if (g >= n) {
                    exhausted = true;
                } else {
                    cur = tword[g];
                    if (othc::task_final(cur)) {
                        done = true;  // one path as it stands
                    } else {
                        const ulonglong2 b = tpos[g];  // x to move
                        othc::start(L, b.x, b.y, (int)othc::task_rem(cur));
                    }
                }
            }
        }
        if (L.depth >= 0) {
            othc::advance<DeviceRules>(L, stk, a.limit);
            if (L.depth < 0) {
                done = true;
                count = L.count;  // (0 at the limit)
                visited = L.nodes;
                if (L.status == othc::kLimit) a.limitf[othc::task_index(cur)] = 1u;  // the finish kernel clears the counts
            }
        }
        if (__ballot(done)) {
            const u64 key = cur & kKeyMask;
            wave_flush(a, pend, done && pend.key != kNoKey && pend.key != key, lane);
            if (done) {
                if (pend.key == kNoKey) {
                    pend.key = key;
                    pend.leaves = 0;
                    pend.nodes = 0;
                }
                pend.leaves += count;
                pend.nodes += visited;
            }
        }
    }
    wave_flush(a, pend, pend.key != kNoKey, lane);
}

// ---- finish ----

struct FinishArgs {
    const u64* boards;
    const uint8_t* depths;
    const u32* limitf;
    unsigned long long* leaves;
    unsigned long long* divide;
    uint8_t* status;
    u64 n;
};

// a wave per position: lane s owns column s of the row
__global__ __launch_bounds__(kBlock) void perft_finish(FinishArgs a) {
    const u64 i = (u64)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
    if (i >= a.n) return;
    const u32 s = threadIdx.x & 63u;
    const bool limit = a.limitf[i] != 0;
    if (limit && a.divide) a.divide[i * 64 + s] = 0;
    if (s != 0) return;
    if (limit && a.leaves) a.leaves[i] = 0;
    if (a.status) {
        const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.boards)[i];
        a.status[i] = (b.x & b.y)                                   ? OTHC_INVALID
                      : (a.depths && a.depths[i] > OTHC_MAX_DEPTH)  ? OTHC_BADDEPTH
                      : limit                                       ? OTHC_LIMIT
                                                                    : OTHC_COUNTED;
    }
}

unsigned blocks_for(int64_t items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

othd::ResidentBlocks g_resident;  // perft_count_kernel's
othd::ResidentBlocks g_expand;    // perft_expand's

int count_grid(int64_t items) {
    return othd::launch_grid(g_resident, reinterpret_cast<const void*>(perft_count_kernel), kCountBlock, items,
                             "OTH_PERFT_BLOCKS");
}

}  // namespace

extern "C" {

int64_t othc_perft_scratch_bytes(int64_t n, int64_t max_tasks) {
    if (n < 0 || max_tasks < 0 || n > OTHC_MAX_TASKS || max_tasks > OTHC_MAX_TASKS) return OTH_EINVAL;
    const int64_t cap = std::max<int64_t>(std::max(max_tasks, n), 1);
    return flags_bytes(n) + 2 * kTaskBytes * cap;
}

int othc_perft_grid(int64_t n) {
    return othd::grid_answer(n, [] { return count_grid((int64_t)OTHC_MAX_TASKS); });
}

int othc_perft(const uint64_t* boards, const uint8_t* turn, int depth, const uint8_t* depths, int split,
               uint32_t node_limit, uint64_t* leaves, uint64_t* divide, uint8_t* status, uint64_t* nodes,
               void* scratch, int64_t scratch_bytes, uint64_t* work, int64_t n, void* stream) {
    if (n < 0 || n > OTHC_MAX_TASKS || !work || depth < 0 || depth > OTHC_MAX_DEPTH || split < 0 ||
        split > OTHC_MAX_SPLIT)
        return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    if (!boards || !scratch || ((uintptr_t)scratch & 15) || scratch_bytes < flags_bytes(n)) return OTH_EINVAL;
    const int64_t cap = std::min<int64_t>((scratch_bytes - flags_bytes(n)) / (2 * kTaskBytes), OTHC_MAX_TASKS);
    if (cap < n || (divide && cap < OTHC_ROOT_SLOTS * n)) return OTH_EINVAL;
    const int levels = std::max(split, divide ? 1 : 0);
    // the count kernel's tasks are the device's to know: about ten per task and level, within the list
    int64_t items = n;
    for (int k = 0; k < levels && items < cap; k++) items *= 10;
    const int grid = count_grid(std::min(items, cap));
    const int egrid = levels ? othd::launch_grid(g_expand, reinterpret_cast<const void*>(perft_expand), kBlock, cap,
                                                 "OTH_PERFT_BLOCKS")
                             : 1;
    if (grid <= 0 || egrid <= 0) return status_of(hipErrorInvalidDevice);
    const Scratch s = scratch_of(scratch, n, cap);
    hipStream_t q = (hipStream_t)stream;
    int rc = status_of(hipMemsetAsync(scratch, 0, (size_t)s.clear_bytes, q));
    if (rc == OTH_OK && leaves) rc = status_of(hipMemsetAsync(leaves, 0, (size_t)n * 8, q));
    if (rc == OTH_OK && divide) rc = status_of(hipMemsetAsync(divide, 0, (size_t)n * 512, q));
    if (rc == OTH_OK && nodes) rc = status_of(hipMemsetAsync(nodes, 0, (size_t)n * 8, q));
    if (rc != OTH_OK) return rc;
    RootArgs r;
    r.boards = boards;
    r.turn = turn;
    r.depths = depths;
    r.count = s.count;
    r.pos = s.pos[0];
    r.word = s.word[0];
    r.n = (u64)n;
    r.depth = depth;
    perft_roots<<<blocks_for(n, kBlock), kBlock, 0, q>>>(r);
    rc = status_of(hipGetLastError());
    if (rc != OTH_OK) return rc;
    for (int k = 1; k <= levels; k++) {
        ExpandArgs e;
        e.src_count = s.count + (k - 1);
        e.dst_count = s.count + k;
        e.src_void = k > 1 ? s.voidf + (k - 1) : nullptr;
        e.dst_void = s.voidf + k;
        e.src_pos = s.pos[(k - 1) & 1];
        e.src_word = s.word[(k - 1) & 1];
        e.dst_pos = s.pos[k & 1];
        e.dst_word = s.word[k & 1];
        e.cap = (u64)cap;
        perft_expand<<<(unsigned)egrid, kBlock, 0, q>>>(e);
        rc = status_of(hipGetLastError());
        if (rc != OTH_OK) return rc;
    }
    CountArgs c;
    c.count = s.count;
    c.voidf = s.voidf;
    for (int k = 0; k < 2; k++) {
        c.pos[k] = s.pos[k];
        c.word[k] = s.word[k];
    }
    c.leaves = reinterpret_cast<unsigned long long*>(leaves);
    c.divide = reinterpret_cast<unsigned long long*>(divide);
    c.nodes = reinterpret_cast<unsigned long long*>(nodes);
    c.limitf = s.limitf;
    c.work = reinterpret_cast<unsigned long long*>(work);
    c.limit = node_limit ? node_limit : OTHC_DEFAULT_NODE_LIMIT;
    c.levels = levels;
    perft_count_kernel<<<(unsigned)grid, kCountBlock, 0, q>>>(c);
    rc = status_of(hipGetLastError());
    if (rc != OTH_OK) return rc;
    if (!leaves && !divide && !status) return OTH_OK;
    FinishArgs f;
    f.boards = boards;
    f.depths = depths;
    f.limitf = s.limitf;
    f.leaves = reinterpret_cast<unsigned long long*>(leaves);
    f.divide = reinterpret_cast<unsigned long long*>(divide);
    f.status = status;
    f.n = (u64)n;
    perft_finish<<<blocks_for(n, kBlock / 64), kBlock, 0, q>>>(f);
    return status_of(hipGetLastError());
}

}  // extern "C"
