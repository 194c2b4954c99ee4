// solve_tree.hip — the split endgame solver for gfx950: one position's exact
// alpha-beta tree over the whole device (include/othello_solve_tree.h,
// DESIGN.md §17).  tree.hip's three launches with the solver's semantics:
//   1. split_solve_expand, one block per position: builds the top of the tree
//      in the position's slab round by round (solve_tree_core.hpp) until every
//      node has at most task_empties empties, children counted by popcounts and
//      placed by a block scan so that they lie in parent order, backs the final
//      nodes' values up, lists the tasks and writes their count;
//   2. split_solve_prefix, one block: the exclusive sum of the task counts;
//   3. split_solve_tasks: solve.hip's persistent loop (one-wave blocks, frames
//      [depth][field][lane] in LDS, the refill protocol off the caller's work
//      word unchanged).  A lane takes a task, derives its window from the state
//      words of its ancestors, runs oths::advance() until the task ends and
//      folds the result into the tree; the lane that completes the root emits
//      the position's answer.
// With order = 1 the third launch is split_solve_tasks_ordered: the same loop
// around solve_order_core.hpp's advance_ordered().
// With a transposition table (include/othello_solve_hash.h) the
// third launch is split_solve_tasks_hashed<ordered>: the same loop around
// solve_hash_core.hpp's machines, which probe and store in the caller's table.
// With a root window (include/othello_solve_window.h) the
// expansion keeps each position's window in its header and the third launch is
// split_window_tasks<ordered, hashed>: the same loop, every task's window
// derived under the root's own and the root's answer clamped into it.
//
// What one block writes and another reads inside the task launch is the state
// word of a node and the position's node counter, both touched by agent-scope
// atomics only; the immutable node fields cross a kernel boundary.  No lane
// waits for another: every loop is bounded by the tree's height, by the
// children of one node or by node_limit.
#include "../../include/othello_solve.h"
#include "../../include/othello_solve_hash.h"
#include "../../include/othello_solve_tree.h"
#include "../../include/othello_solve_window.h"
#include "device_common.hpp"
#include "solve_hash_core.hpp"
#include "solve_order_core.hpp"
#include "solve_tree_core.hpp"

static_assert(OTHE_MAX_EMPTIES == othe::kMaxEmpties && OTHE_NOROOM == othe::kNoRoom &&
                  OTHE_MIN_NODES == othe::kMinNodes && OTHS_MAX_EMPTIES == oths::kMaxEmpties,
              "header and core disagree");
static_assert(OTHS_SKIPPED == oths::kSkipped && OTHS_SOLVED == oths::kSolved && OTHS_INVALID == oths::kInvalid &&
                  OTHS_LIMIT == oths::kLimit && OTHS_NO_MOVE == oths::kNoMove && OTH_PASS == oths::kPassMove,
              "header and core disagree");
static_assert(OTHH_MIN_BITS == othh::kMinBits && OTHH_MAX_BITS == othh::kMaxBits &&
                  OTHH_MIN_EMPTIES_LO == othh::kMinGate && OTHH_MIN_EMPTIES_HI == othh::kMaxGate &&
                  OTHH_DEFAULT_MIN_EMPTIES == othh::kDefaultGate && OTHH_ENTRY_BYTES == othh::kEntryBytes,
              "header and core disagree");

static_assert(OTHS_BADWINDOW == oths::kBadWindow && OTHW_ALPHA_MIN == -othe::kInf && OTHW_BETA_MAX == othe::kInf &&
                  oths::kInf == othe::kInf,
              "header and core disagree");

namespace {

using othe::Node;
using othe::u32;
using othe::u64;

constexpr int kTaskBlock = 64;     // one wave
constexpr int kExpandBlock = 256;
// true: a task's window comes from the state words as they are when it starts;
// false: from the expansion's snapshot
constexpr bool kShareBounds = true;

using othd::DeviceAtomics;
using othd::DeviceRules;
using othd::kRefillMin;
using othd::status_of;
using LdsStack = othd::LdsStack7<kTaskBlock>;
static_assert(LdsStack::kFields == oths::kFields, "the frame's words");

// per position, beside its slab
struct PosHdr {
    unsigned long long nodes;  // the expansion's, then + every task's (agent atomics in the task launch)
    u32 ntasks;
    u32 window;  // the root's (othe::pack_window), written by the expansion, read by split_window_tasks
};

// the caller's scratch, cut up: task prefix [n + 1], headers [n], task lists
// [n][npp], slabs [n][npp]
struct Scratch {
    u64* tbase;
    PosHdr* hdr;
    u32* tasks;
    Node* nodes;
};

inline int64_t round64(int64_t x) { return (x + 63) & ~(int64_t)63; }

inline int64_t scratch_layout(int64_t n, int64_t npp, void* base, Scratch* s) {
    char* p = static_cast<char*>(base);
    int64_t off = 0;
    if (s) s->tbase = reinterpret_cast<u64*>(p + off);
    off += round64((n + 1) * 8);
    if (s) s->hdr = reinterpret_cast<PosHdr*>(p + off);
    off += round64(n * (int64_t)sizeof(PosHdr));
    if (s) s->tasks = reinterpret_cast<u32*>(p + off);
    off += round64(n * npp * 4);
    if (s) s->nodes = reinterpret_cast<Node*>(p + off);
    off += n * npp * (int64_t)sizeof(Node);
    return off;
}

struct Outputs {
    int8_t* value;
    uint8_t* best_move;
    uint8_t* status;
    u32* nodes;
};

__device__ __forceinline__ void emit(const Outputs& o, u64 i, int value, u32 mv, u32 status, u64 nodes) {
    if (o.value) o.value[i] = (int8_t)value;
    if (o.best_move) o.best_move[i] = (uint8_t)mv;
    if (o.status) o.status[i] = (uint8_t)status;
    if (o.nodes) o.nodes[i] = nodes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)nodes;
}

// ------------------------------------------------------------------ expansion
struct ExpandArgs {
    const u64* boards;
    const uint8_t* turn;
    Outputs out;
    Scratch s;
    u32 npp;
    int max_empties;
    int task_empties;
    // each position's root window (othw_solve_split), NULL = -65 / 65 everywhere
    const int8_t* alpha;
    const int8_t* beta;
};

// inclusive block scan of one value per thread; returns the thread's inclusive
// sum, `total` the block's.  Ends with the block in step.
__device__ __forceinline__ u32 block_scan(u32* buf, u32 v, u32& total) {
    const u32 tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
#pragma unroll
    for (u32 d = 1; d < (u32)kExpandBlock; d <<= 1) {
        const u32 add = tid >= d ? buf[tid - d] : 0u;
        __syncthreads();
        buf[tid] += add;
        __syncthreads();
    }
    const u32 incl = buf[tid];
    total = buf[kExpandBlock - 1];
    __syncthreads();
    return incl;
}

__global__ __launch_bounds__(kExpandBlock) void split_solve_expand(ExpandArgs a) {
    __shared__ u32 scan[kExpandBlock];
    __shared__ u32 lvl[othe::kMaxRounds + 2];  // round r's nodes are [lvl[r], lvl[r + 1])
    __shared__ u32 acc;
    const u32 tid = threadIdx.x;
    const u64 pos = blockIdx.x;
    Node* slab = a.s.nodes + pos * a.npp;
    u32* tasks = a.s.tasks + pos * a.npp;
    PosHdr* hdr = a.s.hdr + pos;
    const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.boards)[pos];
    u32 cls = oths::classify(b.x, b.y, 64 - __popcll(b.x | b.y), a.max_empties);
    const int ra = a.alpha ? (int)a.alpha[pos] : -othe::kInf;
    const int rb = a.beta ? (int)a.beta[pos] : othe::kInf;
    if (cls == oths::kSolved && !oths::window_ok(ra, rb)) cls = oths::kBadWindow;
    if (cls != oths::kSolved) {  // (uniform over the block)
        if (tid == 0) {
            emit(a.out, pos, 0, oths::kNoMove, cls, 0);
            hdr->nodes = 0;
            hdr->ntasks = 0;
            hdr->window = othe::pack_window(-othe::kInf, othe::kInf);
        }
        return;
    }
    if (tid == 0) {
        const bool white = a.turn && a.turn[pos] == OTH_WHITE;
        othe::make_node<DeviceRules>(slab[0], white ? b.y : b.x, white ? b.x : b.y, -1, oths::kNoMove);
        lvl[0] = 0;
        lvl[1] = 1;
        acc = 0;
    }
    __syncthreads();
    u32 begin = 0, end = 1;
    int rounds = 0;
    while (rounds < othe::kMaxRounds) {
        // a round is made whole or not at all
        u32 mine = 0;
        for (u32 i = begin + tid; i < end; i += kExpandBlock)
            mine += othe::child_count<DeviceRules>(slab[i], a.task_empties);
        if (mine) atomicAdd(&acc, mine);
        __syncthreads();
        const u32 total = acc;
        __syncthreads();
        if (tid == 0) acc = 0;
        if (total == 0 || (u64)end + total > (u64)a.npp) break;
        u32 running = end;
        for (u32 tile = begin; tile < end; tile += kExpandBlock) {
            const u32 i = tile + tid;
            const u32 c = i < end ? othe::child_count<DeviceRules>(slab[i], a.task_empties) : 0u;
            u32 tile_total;
            const u32 incl = block_scan(scan, c, tile_total);
            if (c) othe::expand<DeviceRules>(slab, i, running + incl - c, c);
            running += tile_total;
        }
        begin = end;
        end += total;
        rounds++;
        if (tid == 0) lvl[rounds + 1] = end;
        __syncthreads();
    }
    __syncthreads();
    // back the values known now up, deepest round first: final nodes, and nodes
    // all of whose children are done
    for (int r = rounds; r >= 1; r--) {
        const u32 lo = lvl[r], hi = lvl[r + 1];
        for (u32 i = lo + tid; i < hi; i += kExpandBlock) {
            const u64 w = DeviceAtomics::load(&slab[i].state);
            if ((slab[i].flags & othe::kFinal) || (slab[i].nchild && othe::count_of(w) == 0))
                othe::fold<DeviceAtomics>(slab, (u32)slab[i].parent, othe::best_of(w), 0);
        }
        __syncthreads();
    }
    for (u32 i = tid; i < end; i += kExpandBlock) slab[i].snap = othe::best_of(DeviceAtomics::load(&slab[i].state));
    // the tasks, in slab order: the order the sequential search would meet them
    u32 ntasks = 0, deep = 0;
    for (u32 tile = 0; tile < end; tile += kExpandBlock) {
        const u32 i = tile + tid;
        const u32 t = i < end && othe::is_task(slab[i]) ? 1u : 0u;
        if (t && slab[i].emp > oths::kMaxEmpties) deep = 1;
        u32 tile_total;
        const u32 incl = block_scan(scan, t, tile_total);
        if (t) tasks[ntasks + incl - 1] = i;
        ntasks += tile_total;
    }
    if (deep) atomicOr(&acc, 1u);
    __syncthreads();
    if (tid == 0) {
        hdr->nodes = end - 1;
        if (acc) {  // the slab is too small for this position at this task size
            emit(a.out, pos, 0, oths::kNoMove, othe::kNoRoom, end - 1);
            ntasks = 0;
        } else if (ntasks == 0) {  // the game ends inside the expanded plies everywhere
            int value;
            u32 mv, st;
            othe::root_result_window<DeviceAtomics>(slab, value, mv, st, ra, rb);
            emit(a.out, pos, value, mv, st, end - 1);
        }
        hdr->ntasks = ntasks;
        hdr->window = othe::pack_window(ra, rb);
    }
}

// ------------------------------------------------------------------ prefix
__global__ __launch_bounds__(kExpandBlock) void split_solve_prefix(Scratch s, u64 n) {
    __shared__ u32 scan[kExpandBlock];
    u64 running = 0;
    for (u64 tile = 0; tile < n; tile += kExpandBlock) {
        const u64 i = tile + threadIdx.x;
        const u32 c = i < n ? s.hdr[i].ntasks : 0u;
        u32 tile_total;
        const u32 incl = block_scan(scan, c, tile_total);
        if (i < n) s.tbase[i] = running + incl - c;
        running += tile_total;
    }
    if (threadIdx.x == 0) s.tbase[n] = running;
}

// ------------------------------------------------------------------ tasks
struct TaskArgs {
    Outputs out;
    Scratch s;
    unsigned long long* work;
    u64 n;
    u64 lanes;  // of the grid: with the task count, what the launch's requests add up to
    u32 npp;
    u32 limit;
};

// The persistent loop of the task launch.  It is written out twice:
// split_solve_tasks_ordered below is this text with the scoring state Q beside
// the lane's L and solve_order_core.hpp's machine inside a task, and a change to one is
// a change to both.  search.hip's and play.hip's pairs are instances of one
// body; these are not, because a kernel that calls its loop compiles to other
// code than a kernel that is its loop (DESIGN.md §16 has the comparison that
// decides such things).
__global__ __launch_bounds__(kTaskBlock) void split_solve_tasks(TaskArgs a) {
    __shared__ u32 frames[oths::kFrames * oths::kFields * kTaskBlock];
    const u32 lane = threadIdx.x;
    const u64 ntasks = a.s.tbase[a.n];
    const u64 total = ntasks + a.lanes;
    LdsStack stk{frames + lane};
    oths::Lane L;
    L.depth = -1;
    u64 pos = 0;
    u32 node = 0;
    bool exhausted = false;  // the lane has made its failing request
    for (;;) {
        const bool idle = L.depth < 0;
        const bool want = idle && !exhausted;
        const u64 wantm = __ballot(want);
        const u64 busym = __ballot(!idle);
        if ((wantm | busym) == 0) break;
        const u64 cnt = (u64)__popcll(wantm);
        bool done = false;  // the lane's task ended in this turn of the loop
        int v = 0;
        u64 lim = 0;
        u32 spent = 0;
        if (wantm != 0 && ((int)cnt >= kRefillMin || busym == 0)) {
            const u64 g = othd::take(a.work, total, wantm, cnt, lane);
            if (want) {
                if (g >= ntasks) {
                    exhausted = true;
                } else {
                    u64 lo = 0, hi = a.n;  // the last position whose first task is <= g
                    while (hi - lo > 1) {
                        const u64 mid = (lo + hi) >> 1;
                        if (a.s.tbase[mid] <= g) lo = mid; else hi = mid;
                    }
                    pos = lo;
                    node = a.s.tasks[pos * a.npp + (g - a.s.tbase[pos])];
                    Node* slab = a.s.nodes + pos * a.npp;
                    int alpha, beta;
                    othe::window<DeviceAtomics>(slab, node, kShareBounds, alpha, beta);
                    if (alpha >= beta) {  // cut off before it began: it reports its beta
                        done = true;
                        v = beta;
                    } else {
                        othe::start_task(L, slab[node], alpha, beta);
                    }
                }
            }
        }
        if (L.depth >= 0) {
            oths::advance<DeviceRules>(L, stk, a.limit);
            if (L.depth < 0) {
                done = true;
                v = L.value;
                lim = L.status == oths::kLimit ? othe::kLimitBit : 0ull;
                spent = L.nodes;
            }
        }
        if (done) {
            Node* slab = a.s.nodes + pos * a.npp;
            PosHdr* hdr = a.s.hdr + pos;
            const u64 before = __hip_atomic_fetch_add(&hdr->nodes, (unsigned long long)spent, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("" ::"v"(before) : "memory");
            if (othe::fold_up<DeviceAtomics>(slab, node, v, lim)) {
                int value;
                u32 mv, st;
                othe::root_result<DeviceAtomics>(slab, value, mv, st);
                emit(a.out, pos, value, mv, st,
                     __hip_atomic_load(&hdr->nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
        }
    }
}

__global__ __launch_bounds__(kTaskBlock) void split_solve_tasks_ordered(TaskArgs a) {
    __shared__ u32 frames[oths::kFrames * oths::kFields * kTaskBlock];
    const u32 lane = threadIdx.x;
    const u64 ntasks = a.s.tbase[a.n];
    const u64 total = ntasks + a.lanes;
    LdsStack stk{frames + lane};
    oths::Lane L;
    L.depth = -1;
    othm::Order Q;
    othm::order_reset(Q);
    u64 pos = 0;
    u32 node = 0;
    bool exhausted = false;  // the lane has made its failing request
    for (;;) {
        const bool idle = L.depth < 0;
        const bool want = idle && !exhausted;
        const u64 wantm = __ballot(want);
        const u64 busym = __ballot(!idle);
        if ((wantm | busym) == 0) break;
        const u64 cnt = (u64)__popcll(wantm);
        bool done = false;  // the lane's task ended in this turn of the loop
        int v = 0;
        u64 lim = 0;
        u32 spent = 0;
        if (wantm != 0 && ((int)cnt >= kRefillMin || busym == 0)) {
            const u64 g = othd::take(a.work, total, wantm, cnt, lane);
            if (want) {
                if (g >= ntasks) {
                    exhausted = true;
                } else {
                    u64 lo = 0, hi = a.n;  // the last position whose first task is <= g
                    while (hi - lo > 1) {
                        const u64 mid = (lo + hi) >> 1;
                        if (a.s.tbase[mid] <= g) lo = mid; else hi = mid;
                    }
                    pos = lo;
                    node = a.s.tasks[pos * a.npp + (g - a.s.tbase[pos])];
                    Node* slab = a.s.nodes + pos * a.npp;
                    int alpha, beta;
                    othe::window<DeviceAtomics>(slab, node, kShareBounds, alpha, beta);
                    if (alpha >= beta) {  // cut off before it began: it reports its beta
                        done = true;
                        v = beta;
                    } else {
                        othe::start_task(L, slab[node], alpha, beta);
                        othm::order_reset(Q);
                    }
                }
            }
        }
        if (L.depth >= 0) {
            oths::advance_ordered<DeviceRules>(L, Q, stk, a.limit);
            if (L.depth < 0) {
                done = true;
                v = L.value;
                lim = L.status == oths::kLimit ? othe::kLimitBit : 0ull;
                spent = L.nodes;
            }
        }
        if (done) {
            Node* slab = a.s.nodes + pos * a.npp;
            PosHdr* hdr = a.s.hdr + pos;
            const u64 before = __hip_atomic_fetch_add(&hdr->nodes, (unsigned long long)spent, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("" ::"v"(before) : "memory");
            if (othe::fold_up<DeviceAtomics>(slab, node, v, lim)) {
                int value;
                u32 mv, st;
                othe::root_result<DeviceAtomics>(slab, value, mv, st);
                emit(a.out, pos, value, mv, st,
                     __hip_atomic_load(&hdr->nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
        }
    }
}

// ------------------------------------------------------------------ tasks with the table
// solve_hash_core.hpp's atomics policy on the device.  Every word of the table
// is read and written by agent-scope atomics on global (address space 1)
// pointers: they bypass the CU's L1, which another CU's stores never refresh,
// and reach the memory all XCDs share.  The orderings are agent-scope fences
// around relaxed accesses.
struct DeviceHashAtomics {
    typedef __attribute__((address_space(1))) unsigned long long gu64;
    static __device__ __forceinline__ gu64* g(u64* p) { return (gu64*)(p); }
    static __device__ __forceinline__ u64 load(u64* p) {
        return __hip_atomic_load(g(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ u64 seq_load(u64* p) { return load(p); }   // read_fence() makes it an acquire
    static __device__ __forceinline__ u64 data_load(u64* p) { return load(p); }  // read_fence() keeps seq's second load behind it
    static __device__ __forceinline__ void read_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }
    static __device__ __forceinline__ bool claim(u64* p, u64 expected, u64 desired) {
        unsigned long long e = expected;
        const bool won = __hip_atomic_compare_exchange_strong(g(p), &e, (unsigned long long)desired, __ATOMIC_RELAXED,
                                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // acquire: the earlier writers' words; release: the claim before this writer's words
        if (won) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
        return won;
    }
    static __device__ __forceinline__ void data_store(u64* p, u64 v) {
        __hip_atomic_store(g(p), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ void publish(u64* p, u64 v) {
        __hip_atomic_store(g(p), (unsigned long long)v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// split_solve_tasks' and split_solve_tasks_ordered's persistent loop, the
// refill protocol and the fold unchanged, around solve_hash_core.hpp's
// machines.  One body for both orders: these kernels have no earlier code to
// keep.
template <bool kOrdered>
__global__ __launch_bounds__(kTaskBlock) void split_solve_tasks_hashed(TaskArgs a, othh::Table tab) {
    __shared__ u32 frames[oths::kFrames * oths::kFields * kTaskBlock];
    const u32 lane = threadIdx.x;
    const u64 ntasks = a.s.tbase[a.n];
    const u64 total = ntasks + a.lanes;
    LdsStack stk{frames + lane};
    oths::Lane L;
    L.depth = -1;
    othm::Order Q;
    othm::order_reset(Q);
    u64 pos = 0;
    u32 node = 0;
    bool exhausted = false;  // the lane has made its failing request
    for (;;) {
        const bool idle = L.depth < 0;
        const bool want = idle && !exhausted;
        const u64 wantm = __ballot(want);
        const u64 busym = __ballot(!idle);
        if ((wantm | busym) == 0) break;
        const u64 cnt = (u64)__popcll(wantm);
        bool done = false;  // the lane's task ended in this turn of the loop
        int v = 0;
        u64 lim = 0;
        u32 spent = 0;
        if (wantm != 0 && ((int)cnt >= kRefillMin || busym == 0)) {
            const u64 g = othd::take(a.work, total, wantm, cnt, lane);
            if (want) {
                if (g >= ntasks) {
                    exhausted = true;
                } else {
                    u64 lo = 0, hi = a.n;  // the last position whose first task is <= g
                    while (hi - lo > 1) {
                        const u64 mid = (lo + hi) >> 1;
                        if (a.s.tbase[mid] <= g) lo = mid; else hi = mid;
                    }
                    pos = lo;
                    node = a.s.tasks[pos * a.npp + (g - a.s.tbase[pos])];
                    Node* slab = a.s.nodes + pos * a.npp;
                    int alpha, beta;
                    othe::window<DeviceAtomics>(slab, node, kShareBounds, alpha, beta);
                    if (alpha >= beta) {  // cut off before it began: it reports its beta
                        done = true;
                        v = beta;
                    } else {
                        othe::start_task(L, slab[node], alpha, beta);
                        othm::order_reset(Q);
                    }
                }
            }
        }
        if (L.depth >= 0) {
            if constexpr (kOrdered)
                othh::advance_ordered_hashed<DeviceRules, DeviceHashAtomics>(L, Q, stk, tab, a.limit);
            else
                othh::advance_hashed<DeviceRules, DeviceHashAtomics>(L, stk, tab, a.limit);
            if (L.depth < 0) {
                done = true;
                v = L.value;
                lim = L.status == oths::kLimit ? othe::kLimitBit : 0ull;
                spent = L.nodes;
            }
        }
        if (done) {
            Node* slab = a.s.nodes + pos * a.npp;
            PosHdr* hdr = a.s.hdr + pos;
            const u64 before = __hip_atomic_fetch_add(&hdr->nodes, (unsigned long long)spent, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("" ::"v"(before) : "memory");
            if (othe::fold_up<DeviceAtomics>(slab, node, v, lim)) {
                int value;
                u32 mv, st;
                othe::root_result<DeviceAtomics>(slab, value, mv, st);
                emit(a.out, pos, value, mv, st,
                     __hip_atomic_load(&hdr->nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
        }
    }
}

// ------------------------------------------------------------------ tasks under a root window
// othw_solve_split's task launch: the loop above once more, with every task's
// window derived under its root's own (the position's header has it) and the
// root's answer clamped into it (solve_tree_core.hpp's window_rooted and
// root_result_window).  One body for the four kernels, plain or
// hashed x either move order: they have no earlier code to keep, and the three
// kernels above, which the calls without a window launch, stay what they were.
template <bool kOrdered, bool kHashed>
__global__ __launch_bounds__(kTaskBlock) void split_window_tasks(TaskArgs a, othh::Table tab) {
    __shared__ u32 frames[oths::kFrames * oths::kFields * kTaskBlock];
    const u32 lane = threadIdx.x;
    const u64 ntasks = a.s.tbase[a.n];
    const u64 total = ntasks + a.lanes;
    LdsStack stk{frames + lane};
    oths::Lane L;
    L.depth = -1;
    othm::Order Q;
    othm::order_reset(Q);
    u64 pos = 0;
    u32 node = 0;
    bool exhausted = false;  // the lane has made its failing request
    for (;;) {
        const bool idle = L.depth < 0;
        const bool want = idle && !exhausted;
        const u64 wantm = __ballot(want);
        const u64 busym = __ballot(!idle);
        if ((wantm | busym) == 0) break;
        const u64 cnt = (u64)__popcll(wantm);
        bool done = false;  // the lane's task ended in this turn of the loop
        int v = 0;
        u64 lim = 0;
        u32 spent = 0;
        if (wantm != 0 && ((int)cnt >= kRefillMin || busym == 0)) {
            const u64 g = othd::take(a.work, total, wantm, cnt, lane);
            if (want) {
                if (g >= ntasks) {
                    exhausted = true;
                } else {
                    u64 lo = 0, hi = a.n;  // the last position whose first task is <= g
                    while (hi - lo > 1) {
                        const u64 mid = (lo + hi) >> 1;
                        if (a.s.tbase[mid] <= g) lo = mid; else hi = mid;
                    }
                    pos = lo;
                    node = a.s.tasks[pos * a.npp + (g - a.s.tbase[pos])];
                    Node* slab = a.s.nodes + pos * a.npp;
                    int alpha, beta;
                    const u32 rw = a.s.hdr[pos].window;
                    othe::window_rooted<DeviceAtomics>(slab, node, kShareBounds, alpha, beta, othe::window_alpha(rw),
                                                       othe::window_beta(rw));
                    if (alpha >= beta) {  // cut off before it began: it reports its beta
                        done = true;
                        v = beta;
                    } else {
                        othe::start_task(L, slab[node], alpha, beta);
                        othm::order_reset(Q);
                    }
                }
            }
        }
        if (L.depth >= 0) {
            if constexpr (kOrdered && kHashed)
                othh::advance_ordered_hashed<DeviceRules, DeviceHashAtomics>(L, Q, stk, tab, a.limit);
            else if constexpr (kHashed)
                othh::advance_hashed<DeviceRules, DeviceHashAtomics>(L, stk, tab, a.limit);
            else if constexpr (kOrdered)
                oths::advance_ordered<DeviceRules>(L, Q, stk, a.limit);
            else
                oths::advance<DeviceRules>(L, stk, a.limit);
            if (L.depth < 0) {
                done = true;
                v = L.value;
                lim = L.status == oths::kLimit ? othe::kLimitBit : 0ull;
                spent = L.nodes;
            }
        }
        if (done) {
            Node* slab = a.s.nodes + pos * a.npp;
            PosHdr* hdr = a.s.hdr + pos;
            const u64 before = __hip_atomic_fetch_add(&hdr->nodes, (unsigned long long)spent, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("" ::"v"(before) : "memory");
            if (othe::fold_up<DeviceAtomics>(slab, node, v, lim)) {
                int value;
                u32 mv, st;
                othe::root_result_window<DeviceAtomics>(slab, value, mv, st, othe::window_alpha(hdr->window),
                                                        othe::window_beta(hdr->window));
                emit(a.out, pos, value, mv, st,
                     __hip_atomic_load(&hdr->nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
        }
    }
}

// one cache for split_solve_tasks (order 0), one for the ordered kernel (1),
// two for their hashed twins, four for the kernels under a root window
othd::ResidentBlocks g_resident[8];

int task_grid(int64_t tasks, int order, bool hashed = false, bool windowed = false) {
    const void* kernel =
        windowed ? (hashed ? (order ? reinterpret_cast<const void*>(split_window_tasks<true, true>)
                                    : reinterpret_cast<const void*>(split_window_tasks<false, true>))
                           : (order ? reinterpret_cast<const void*>(split_window_tasks<true, false>)
                                    : reinterpret_cast<const void*>(split_window_tasks<false, false>)))
        : hashed ? (order ? reinterpret_cast<const void*>(split_solve_tasks_hashed<true>)
                          : reinterpret_cast<const void*>(split_solve_tasks_hashed<false>))
                 : (order ? reinterpret_cast<const void*>(split_solve_tasks_ordered)
                          : reinterpret_cast<const void*>(split_solve_tasks));
    return othd::launch_grid(g_resident[order + (hashed ? 2 : 0) + (windowed ? 4 : 0)], kernel, kTaskBlock, tasks,
                             "OTH_SOLVE_BLOCKS", true);
}

// n * npp, or -1 when the scratch would not fit 2^62 bytes
int64_t slab_nodes(int64_t n, int64_t npp) {
    if (n < 0 || npp < OTHE_MIN_NODES || npp > (1 << 30)) return -1;
    if (n > 0 && npp > ((int64_t)1 << 55) / n) return -1;
    return n * npp;
}

// othe_solve's launches; with a table the task launch is the hashed kernel's,
// and `windowed` (othw_solve_split; alpha / beta NULL: the window's full end)
// the kernels' under a root window
int launch_solve(const uint64_t* boards, const uint8_t* turn, bool windowed, const int8_t* alpha, const int8_t* beta,
                 int max_empties, int task_empties, int order,
                 uint32_t node_limit, int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes, void* scratch,
                 int64_t scratch_bytes, int32_t nodes_per_position, uint64_t* work, int64_t n, const othh::Table* tab,
                 void* stream) {
    if (order < 0 || order > 1) return OTH_EINVAL;
    if (n < 0 || n > 0x7FFFFFFF || !work || (n > 0 && !boards)) return OTH_EINVAL;
    if (max_empties < 0 || max_empties > OTHE_MAX_EMPTIES || task_empties < 1 || task_empties > OTHS_MAX_EMPTIES)
        return OTH_EINVAL;
    const int64_t total_nodes = slab_nodes(n, nodes_per_position);
    if (total_nodes < 0) return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < scratch_layout(n, nodes_per_position, nullptr, nullptr))
        return OTH_EINVAL;
    // a position has no more tasks than its slab holds
    const int grid = task_grid(total_nodes, order, tab != nullptr, windowed);
    if (grid <= 0) return status_of(hipErrorInvalidDevice);
    hipStream_t st = (hipStream_t)stream;
    Outputs out{value, best_move, status, nodes};
    ExpandArgs e;
    e.boards = boards;
    e.turn = turn;
    e.out = out;
    scratch_layout(n, nodes_per_position, scratch, &e.s);
    e.npp = (u32)nodes_per_position;
    e.max_empties = max_empties;
    e.task_empties = task_empties;
    e.alpha = alpha;
    e.beta = beta;
    split_solve_expand<<<(unsigned)n, kExpandBlock, 0, st>>>(e);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return status_of(err);
    split_solve_prefix<<<1, kExpandBlock, 0, st>>>(e.s, (u64)n);
    err = hipGetLastError();
    if (err != hipSuccess) return status_of(err);
    TaskArgs t;
    t.out = out;
    t.s = e.s;
    t.work = reinterpret_cast<unsigned long long*>(work);
    t.n = (u64)n;
    t.lanes = (u64)grid * kTaskBlock;
    t.npp = (u32)nodes_per_position;
    t.limit = node_limit ? node_limit : OTHS_DEFAULT_NODE_LIMIT;
    const othh::Table none{nullptr, 0, 0};
    if (windowed && tab && order)
        split_window_tasks<true, true><<<(unsigned)grid, kTaskBlock, 0, st>>>(t, *tab);
    else if (windowed && tab)
        split_window_tasks<false, true><<<(unsigned)grid, kTaskBlock, 0, st>>>(t, *tab);
    else if (windowed && order)
        split_window_tasks<true, false><<<(unsigned)grid, kTaskBlock, 0, st>>>(t, none);
    else if (windowed)
        split_window_tasks<false, false><<<(unsigned)grid, kTaskBlock, 0, st>>>(t, none);
    else if (tab && order)
        split_solve_tasks_hashed<true><<<(unsigned)grid, kTaskBlock, 0, st>>>(t, *tab);
    else if (tab)
        split_solve_tasks_hashed<false><<<(unsigned)grid, kTaskBlock, 0, st>>>(t, *tab);
    else if (order)
        split_solve_tasks_ordered<<<(unsigned)grid, kTaskBlock, 0, st>>>(t);
    else
        split_solve_tasks<<<(unsigned)grid, kTaskBlock, 0, st>>>(t);
    return status_of(hipGetLastError());
}

// othh_solve_hashed's checks of its table arguments; false: OTH_EINVAL
bool make_table(int hash_bits, int hash_min_empties, void* table, int64_t table_bytes, othh::Table& tab) {
    if (hash_bits < OTHH_MIN_BITS || hash_bits > OTHH_MAX_BITS || hash_min_empties < OTHH_MIN_EMPTIES_LO ||
        hash_min_empties > OTHH_MIN_EMPTIES_HI)
        return false;
    if (!table || ((uintptr_t)table & (OTHH_ENTRY_BYTES - 1)) || table_bytes < ((int64_t)OTHH_ENTRY_BYTES << hash_bits))
        return false;
    tab.e = static_cast<othh::Entry*>(table);
    tab.shift = 64 - hash_bits;
    tab.min_empties = hash_min_empties;
    return true;
}

}  // namespace

extern "C" {

int64_t othe_scratch_bytes(int64_t n, int32_t nodes_per_position) {
    if (slab_nodes(n, nodes_per_position) < 0) return OTH_EINVAL;
    return scratch_layout(n, nodes_per_position, nullptr, nullptr);
}

int othe_solve(const uint64_t* boards, const uint8_t* turn, int max_empties, int task_empties, int order,
               uint32_t node_limit, int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
               void* scratch, int64_t scratch_bytes, int32_t nodes_per_position, uint64_t* work, int64_t n,
               void* stream) {
    return launch_solve(boards, turn, false, nullptr, nullptr, max_empties, task_empties, order, node_limit, value, best_move, status, nodes,
                        scratch, scratch_bytes, nodes_per_position, work, n, nullptr, stream);
}

int64_t othh_hash_bytes(int hash_bits) {
    if (hash_bits < OTHH_MIN_BITS || hash_bits > OTHH_MAX_BITS) return OTH_EINVAL;
    return (int64_t)OTHH_ENTRY_BYTES << hash_bits;
}

int othh_solve_hashed(const uint64_t* boards, const uint8_t* turn, int max_empties, int task_empties, int order,
                      uint32_t node_limit, int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
                      void* scratch, int64_t scratch_bytes, int32_t nodes_per_position, uint64_t* work, int64_t n,
                      int hash_bits, int hash_min_empties, void* table, int64_t table_bytes, void* stream) {
    othh::Table tab;
    if (!make_table(hash_bits, hash_min_empties, table, table_bytes, tab)) return OTH_EINVAL;
    return launch_solve(boards, turn, false, nullptr, nullptr, max_empties, task_empties, order, node_limit, value, best_move, status, nodes,
                        scratch, scratch_bytes, nodes_per_position, work, n, &tab, stream);
}

int othw_solve_split(const uint64_t* boards, const uint8_t* turn, int max_empties, int task_empties, int order,
                     uint32_t node_limit, int8_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
                     void* scratch, int64_t scratch_bytes, int32_t nodes_per_position, uint64_t* work, int64_t n,
                     const int8_t* alpha, const int8_t* beta, int hash_bits, int hash_min_empties, void* table,
                     int64_t table_bytes, void* stream) {
    if (!table && hash_bits == 0)
        return launch_solve(boards, turn, true, alpha, beta, max_empties, task_empties, order, node_limit, value, best_move,
                            status, nodes, scratch, scratch_bytes, nodes_per_position, work, n, nullptr, stream);
    othh::Table tab;
    if (!make_table(hash_bits, hash_min_empties, table, table_bytes, tab)) return OTH_EINVAL;
    return launch_solve(boards, turn, true, alpha, beta, max_empties, task_empties, order, node_limit, value, best_move,
                        status, nodes, scratch, scratch_bytes, nodes_per_position, work, n, &tab, stream);
}

int othe_solve_grid(int64_t tasks) {
    return othd::grid_answer(tasks, [&] { return task_grid(tasks, 0); });
}

}  // extern "C"
