// tree.hip — the split search for gfx950: one position's alpha-beta tree over
// the whole device (include/othello_tree.h).
//
// Three launches on the caller's stream, no host round trip:
//   1. expand_kernel, one block per position: builds the top of the tree in
//      the position's slab round by round (tree_core.hpp), children counted by
//      popcounts and placed by a block scan so that they lie in parent order,
//      backs the final nodes' values up, lists the tasks and writes their count;
//   2. prefix_kernel, one block: the exclusive sum of the task counts, which
//      maps a global task index to (position, task) by a binary search;
//   3. task_kernel: search.hip's persistent loop (one-wave blocks, frames
//      [depth][field][lane] and the widened table in LDS, the refill protocol
//      off the caller's work word unchanged).  A lane takes a task, derives its
//      window from the state words of its ancestors, runs othm::advance() until
//      the task ends and folds the result into the tree; the lane that
//      completes the root emits the position's answer.
//
// With order = 1 (include/othello_order.h) the third launch is
// task_ordered_kernel: the same loop around order_core.hpp's advance_ordered()
// with the root tie rule off; the expansion is the same in both orders.
//
// What one block writes and another reads inside the task launch is the state
// word of a node and the position's node counter, both touched by agent-scope
// atomics only; the immutable node fields cross a kernel boundary.  No lane
// waits for another: every loop is bounded by the tree's height or by the
// children of one node.
#include "../../include/othello_search.h"
#include "../../include/othello_tree.h"
#include "../../include/othello_order.h"
#include "device_common.hpp"
#include "order_core.hpp"
#include "tree_core.hpp"

static_assert(OTHT_MAX_SPLIT == otht::kMaxSplit && OTHT_NOROOM == otht::kNoRoom && OTHT_MIN_NODES == otht::kMinNodes,
              "header and core disagree");
static_assert(OTHM_MAX_DEPTH == othm::kMaxDepth && OTHM_SEARCHED == othm::kSearched &&
                  OTHM_INVALID == othm::kInvalid && OTHM_LIMIT == othm::kLimit && OTHM_NO_MOVE == othm::kNoMove,
              "header and core disagree");

namespace {

using otht::Node;
using otht::u32;
using otht::u64;

constexpr int kTaskBlock = 64;     // one wave
constexpr int kExpandBlock = 256;
// true: a task's window comes from the state words as they are when it starts;
// false: from the expansion's snapshot (tools/diag/tree_snapshot.patch)
constexpr bool kShareBounds = true;

using othd::DeviceAtomics;
using othd::DeviceRules;
using othd::kRefillMin;
using othd::status_of;
using LdsStack = othd::LdsStack9<kTaskBlock>;
static_assert(LdsStack::kFields == othm::kFields, "the frame's words");

// per position, beside its slab
struct PosHdr {
    unsigned long long nodes;  // the expansion's, then + every task's (agent atomics in the task launch)
    u32 ntasks;
    u32 pad;
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
    int32_t* value;
    uint8_t* best_move;
    uint8_t* status;
    u32* nodes;
};

__device__ __forceinline__ void emit(const Outputs& o, u64 i, int value, u32 mv, u32 status, u64 nodes) {
    if (o.value) o.value[i] = value;
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
    int depth;
    int split;
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

__global__ __launch_bounds__(kExpandBlock) void expand_kernel(ExpandArgs a) {
    __shared__ u32 scan[kExpandBlock];
    __shared__ u32 lvl[otht::kMaxRounds + 2];  // round r's nodes are [lvl[r], lvl[r + 1])
    __shared__ u32 acc;
    const u32 tid = threadIdx.x;
    const u64 pos = blockIdx.x;
    Node* slab = a.s.nodes + pos * a.npp;
    u32* tasks = a.s.tasks + pos * a.npp;
    PosHdr* hdr = a.s.hdr + pos;
    const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.boards)[pos];
    if (b.x & b.y) {
        if (tid == 0) {
            emit(a.out, pos, 0, othm::kNoMove, othm::kInvalid, 0);
            hdr->nodes = 0;
            hdr->ntasks = 0;
        }
        return;
    }
    if (tid == 0) {
        const bool white = a.turn && a.turn[pos] == OTH_WHITE;
        otht::make_node<DeviceRules>(slab[0], white ? b.y : b.x, white ? b.x : b.y, -1, othm::kNoMove, a.depth,
                                     otht::kSideRoot);
        lvl[0] = 0;
        lvl[1] = 1;
        acc = 0;
    }
    __syncthreads();
    const int target = a.depth - a.split;
    u32 begin = 0, end = 1;
    int rounds = 0;
    while (rounds < otht::kMaxRounds) {
        // a round is made whole or not at all
        u32 mine = 0;
        for (u32 i = begin + tid; i < end; i += kExpandBlock) mine += otht::child_count<DeviceRules>(slab[i], target);
        if (mine) atomicAdd(&acc, mine);
        __syncthreads();
        const u32 total = acc;
        __syncthreads();
        if (tid == 0) acc = 0;
        if (total == 0 || (u64)end + total > (u64)a.npp) break;
        u32 running = end;
        for (u32 tile = begin; tile < end; tile += kExpandBlock) {
            const u32 i = tile + tid;
            const u32 c = i < end ? otht::child_count<DeviceRules>(slab[i], target) : 0u;
            u32 tile_total;
            const u32 incl = block_scan(scan, c, tile_total);
            if (c) otht::expand<DeviceRules>(slab, i, running + incl - c, c);
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
            if ((slab[i].flags & otht::kFinal) || (slab[i].nchild && otht::count_of(w) == 0))
                otht::fold<DeviceAtomics>(slab, (u32)slab[i].parent, otht::best_of(w), 0);
        }
        __syncthreads();
    }
    for (u32 i = tid; i < end; i += kExpandBlock) slab[i].snap = otht::best_of(DeviceAtomics::load(&slab[i].state));
    // the tasks, in slab order: the order the sequential search would meet them
    u32 ntasks = 0, deep = 0;
    for (u32 tile = 0; tile < end; tile += kExpandBlock) {
        const u32 i = tile + tid;
        const u32 t = i < end && otht::is_task(slab[i]) ? 1u : 0u;
        if (t && slab[i].rem > othm::kMaxDepth) deep = 1;
        u32 tile_total;
        const u32 incl = block_scan(scan, t, tile_total);
        if (t) tasks[ntasks + incl - 1] = i;
        ntasks += tile_total;
    }
    if (deep) atomicOr(&acc, 1u);
    __syncthreads();
    if (tid == 0) {
        hdr->nodes = end - 1;
        if (acc) {  // the slab is too small for this position at this depth
            emit(a.out, pos, 0, othm::kNoMove, otht::kNoRoom, end - 1);
            ntasks = 0;
        } else if (ntasks == 0) {  // the game ends inside the split plies everywhere
            int value;
            u32 mv, st;
            otht::root_result<DeviceAtomics>(slab, value, mv, st);
            emit(a.out, pos, value, mv, st, end - 1);
        }
        hdr->ntasks = ntasks;
    }
}

// ------------------------------------------------------------------ prefix
__global__ __launch_bounds__(kExpandBlock) void prefix_kernel(Scratch s, u64 n) {
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
    int8_t w[OTH_EVAL_WEIGHTS];
};

// The persistent loop of the task launch.  It is written out twice:
// task_ordered_kernel below is this text with the scoring state Q beside
// the lane's L and order_core.hpp's machine inside a task, and a change to one is
// a change to both.  search.hip's and play.hip's pairs are instances of one
// body; these are not, because a kernel that calls its loop compiles to other
// code than a kernel that is its loop (DESIGN.md §16 has the comparison that
// decides such things).
__global__ __launch_bounds__(kTaskBlock) void task_kernel(TaskArgs a) {
    __shared__ u32 frames[othm::kFrames * othm::kFields * kTaskBlock];
    __shared__ int table[othm::kEvalTable];
    const u32 lane = threadIdx.x;
    if (lane < (u32)othm::kEvalTable) othm::widen_weight(a.w, (int)lane, table);
    __syncthreads();
    const u64 ntasks = a.s.tbase[a.n];
    const u64 total = ntasks + a.lanes;
    LdsStack stk{frames + lane};
    othm::Lane L;
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
                    otht::window<DeviceAtomics>(slab, node, kShareBounds, alpha, beta);
                    if (alpha >= beta) {  // cut off before it began: it reports its beta
                        done = true;
                        v = beta;
                    } else {
                        otht::start_task(L, slab[node], alpha, beta);
                    }
                }
            }
        }
        if (L.depth >= 0) {
            othm::advance<DeviceRules>(L, stk, table, a.limit);
            if (L.depth < 0) {
                done = true;
                v = L.value;
                lim = L.status == othm::kLimit ? otht::kLimitBit : 0ull;
                spent = L.nodes;
            }
        }
        if (done) {
            Node* slab = a.s.nodes + pos * a.npp;
            PosHdr* hdr = a.s.hdr + pos;
            const u64 before = __hip_atomic_fetch_add(&hdr->nodes, (unsigned long long)spent, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("" ::"v"(before) : "memory");
            if (otht::fold_up<DeviceAtomics>(slab, node, v, lim)) {
                int value;
                u32 mv, st;
                otht::root_result<DeviceAtomics>(slab, value, mv, st);
                emit(a.out, pos, value, mv, st,
                     __hip_atomic_load(&hdr->nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
        }
    }
}

__global__ __launch_bounds__(kTaskBlock) void task_ordered_kernel(TaskArgs a) {
    __shared__ u32 frames[othm::kFrames * othm::kFields * kTaskBlock];
    __shared__ int table[othm::kEvalTable];
    const u32 lane = threadIdx.x;
    if (lane < (u32)othm::kEvalTable) othm::widen_weight(a.w, (int)lane, table);
    __syncthreads();
    const u64 ntasks = a.s.tbase[a.n];
    const u64 total = ntasks + a.lanes;
    LdsStack stk{frames + lane};
    othm::Lane L;
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
                    otht::window<DeviceAtomics>(slab, node, kShareBounds, alpha, beta);
                    if (alpha >= beta) {  // cut off before it began: it reports its beta
                        done = true;
                        v = beta;
                    } else {
                        otht::start_task(L, slab[node], alpha, beta);
                        othm::order_reset(Q);
                    }
                }
            }
        }
        if (L.depth >= 0) {
            othm::advance_ordered<DeviceRules, false>(L, Q, stk, table, a.limit);
            if (L.depth < 0) {
                done = true;
                v = L.value;
                lim = L.status == othm::kLimit ? otht::kLimitBit : 0ull;
                spent = L.nodes;
            }
        }
        if (done) {
            Node* slab = a.s.nodes + pos * a.npp;
            PosHdr* hdr = a.s.hdr + pos;
            const u64 before = __hip_atomic_fetch_add(&hdr->nodes, (unsigned long long)spent, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("" ::"v"(before) : "memory");
            if (otht::fold_up<DeviceAtomics>(slab, node, v, lim)) {
                int value;
                u32 mv, st;
                otht::root_result<DeviceAtomics>(slab, value, mv, st);
                emit(a.out, pos, value, mv, st,
                     __hip_atomic_load(&hdr->nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
        }
    }
}

// one cache for task_kernel (order 0), one for the ordered kernel (1)
othd::ResidentBlocks g_resident[2];

int task_grid(int64_t tasks, int order) {
    const void* kernel = order ? reinterpret_cast<const void*>(task_ordered_kernel)
                               : reinterpret_cast<const void*>(task_kernel);
    return othd::launch_grid(g_resident[order], kernel, kTaskBlock, tasks, "OTH_SEARCH_BLOCKS", true);
}

// n * npp, or -1 when the scratch would not fit 2^62 bytes
int64_t slab_nodes(int64_t n, int64_t npp) {
    if (n < 0 || npp < OTHT_MIN_NODES || npp > (1 << 30)) return -1;
    if (n > 0 && npp > ((int64_t)1 << 55) / n) return -1;
    return n * npp;
}

}  // namespace

extern "C" {

int64_t otht_scratch_bytes(int64_t n, int32_t nodes_per_position) {
    if (slab_nodes(n, nodes_per_position) < 0) return OTH_EINVAL;
    return scratch_layout(n, nodes_per_position, nullptr, nullptr);
}

int otho_tree_ordered(const uint64_t* boards, const uint8_t* turn, int depth, int split, int order,
                      const int8_t* weights, uint32_t node_limit, int32_t* value, uint8_t* best_move, uint8_t* status,
                      uint32_t* nodes, void* scratch, int64_t scratch_bytes, int32_t nodes_per_position,
                      uint64_t* work, int64_t n, void* stream) {
    if (order < 0 || order > OTHO_MAX_ORDER) return OTH_EINVAL;
    if (n < 0 || n > 0x7FFFFFFF || !work || !weights || (n > 0 && !boards)) return OTH_EINVAL;
    if (split < 1 || split > OTHT_MAX_SPLIT || depth <= split || depth > split + OTHM_MAX_DEPTH) return OTH_EINVAL;
    const int64_t total_nodes = slab_nodes(n, nodes_per_position);
    if (total_nodes < 0) return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < scratch_layout(n, nodes_per_position, nullptr, nullptr))
        return OTH_EINVAL;
    // a position has at most 33^split tasks, and no more than its slab holds
    int64_t per = 1;
    for (int k = 0; k < split; k++) per = std::min<int64_t>(per * 33, nodes_per_position);
    const int grid = task_grid(n * per, order);
    if (grid <= 0) return status_of(hipErrorInvalidDevice);
    hipStream_t st = (hipStream_t)stream;
    Outputs out{value, best_move, status, nodes};
    ExpandArgs e;
    e.boards = boards;
    e.turn = turn;
    e.out = out;
    scratch_layout(n, nodes_per_position, scratch, &e.s);
    e.npp = (u32)nodes_per_position;
    e.depth = depth;
    e.split = split;
    expand_kernel<<<(unsigned)n, kExpandBlock, 0, st>>>(e);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return status_of(err);
    prefix_kernel<<<1, kExpandBlock, 0, st>>>(e.s, (u64)n);
    err = hipGetLastError();
    if (err != hipSuccess) return status_of(err);
    TaskArgs t;
    t.out = out;
    t.s = e.s;
    t.work = reinterpret_cast<unsigned long long*>(work);
    t.n = (u64)n;
    t.lanes = (u64)grid * kTaskBlock;
    t.npp = (u32)nodes_per_position;
    t.limit = node_limit ? node_limit : OTHM_DEFAULT_NODE_LIMIT;
    for (int k = 0; k < OTH_EVAL_WEIGHTS; k++) t.w[k] = weights[k];
    if (order)
        task_ordered_kernel<<<(unsigned)grid, kTaskBlock, 0, st>>>(t);
    else
        task_kernel<<<(unsigned)grid, kTaskBlock, 0, st>>>(t);
    return status_of(hipGetLastError());
}

int otht_search(const uint64_t* boards, const uint8_t* turn, int depth, int split, const int8_t* weights,
                uint32_t node_limit, int32_t* value, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
                void* scratch, int64_t scratch_bytes, int32_t nodes_per_position, uint64_t* work, int64_t n,
                void* stream) {
    return otho_tree_ordered(boards, turn, depth, split, 0, weights, node_limit, value, best_move, status, nodes,
                               scratch, scratch_bytes, nodes_per_position, work, n, stream);
}

int otho_tree_ordered_grid(int64_t tasks, int order) {
    if (order < 0 || order > OTHO_MAX_ORDER) return OTH_EINVAL;
    return othd::grid_answer(tasks, [&] { return task_grid(tasks, order); });
}

int otht_search_grid(int64_t tasks) { return otho_tree_ordered_grid(tasks, 0); }

}  // extern "C"
