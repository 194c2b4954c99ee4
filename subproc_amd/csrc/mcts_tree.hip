// mcts_tree.hip — Monte Carlo search trees that persist, for gfx950
// (include/othello_mcts_tree.h): mcts.hip's trees in the caller's
// memory, one slab and one record per tree, with four operations.
//
//   init     a thread per tree: the root and the record;
//   search   mcts.hip's kernel over slab i for tree i: a block is one wave and
//            walks trees b, b + grid, ...; mcts_core.hpp's iterate() from the
//            record's node count and played count, then the rows.  The tree's
//            memory, the wave and the playout are mcts_device.hpp's, the ray
//            and k-th bit tables in LDS as there;
//   rows     the same kernel without the tables and the iterations;
//   advance  a wave per tree: mcts_core.hpp's advance().  The kept subtree is
//            copied breadth first into the slab's second half and back; the
//            places of a turn's children blocks are a wave prefix sum.  Its
//            phases are separated by SlabTree::sync(), the workgroup-scope
//            fence of the search.
// No wave reads another wave's slab or record: nothing atomic, nothing at agent
// scope, no waiting, no scratch memory.  A record that is not READY for this
// max_nodes keeps every kernel away from its slab.
#include "../../include/othello_mcts_tree.h"
#include "mcts_device.hpp"

static_assert(OTHR_READY == OTHU_SEARCHED && OTHR_INVALID == OTHU_INVALID && OTHR_KEEP == OTHU_NO_MOVE &&
                  OTHR_LDS_BYTES == OTHU_LDS_BYTES,
              "the statuses, the move that is none and the LDS are othello_mcts.h's");

namespace {

using namespace oth;
using othd::status_of;
using othud::kBlock;
using othud::MctsRules;
using othud::SlabTree;
using othud::Wave;

struct Record {
    u64 id_base, played;
    u32 nodes, turn, status, max_nodes;
};
static_assert(sizeof(Record) == OTHR_RECORD_BYTES, "the header's record");

struct Trees {
    char* slabs;
    Record* records;
    u32 max_nodes;
    u64 n;
    __device__ __forceinline__ u64 half_bytes() const { return (u64)max_nodes * OTHU_NODE_BYTES; }
    __device__ __forceinline__ SlabTree tree(u64 i) const {
        return othud::slab_tree(slabs + i * 2u * half_bytes(), max_nodes);
    }
    __device__ __forceinline__ SlabTree half(u64 i) const {
        return othud::slab_tree(slabs + (i * 2u + 1u) * half_bytes(), max_nodes);
    }
    // whether a kernel may walk tree i
    __device__ __forceinline__ bool ready(const Record& r) const {
        return r.status == OTHR_READY && r.max_nodes == max_nodes && r.nodes >= 1u && r.nodes <= max_nodes;
    }
};

// ---- init ----
struct InitArgs {
    const u64* boards;
    const uint8_t* turn;
    const u64* id_base;
    u64 game_id0, stride;
    Trees t;
};

__global__ __launch_bounds__(256) void tree_init_kernel(InitArgs a) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.t.n) return;
    const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.boards)[i];
    const bool white = a.turn && a.turn[i] == OTH_WHITE;
    const bool valid = (b.x & b.y) == 0;
    SlabTree tree = a.t.tree(i);
    tree.set_pos(0u, white ? b.y : b.x, white ? b.x : b.y);
    tree.set_stats(0u, 0u, 0u, 0);
    tree.set_link(0u, 0u);
    Record r;
    r.id_base = a.id_base ? a.id_base[i] : a.game_id0 + i * a.stride;
    r.played = 0;
    r.nodes = valid ? 1u : 0u;
    r.turn = white ? OTH_WHITE : OTH_BLACK;
    r.status = valid ? OTHR_READY : OTHR_INVALID;
    r.max_nodes = a.t.max_nodes;
    a.t.records[i] = r;
}

// ---- search and rows ----
struct SearchArgs {
    u32 iterations;
    const u32* per_tree;
    othu::Params p;  // (iterations and game_id0 unused: the record's)
    u32 *visits, *wins;
    int* diffs;
    u32* root_wins;
    int* root_diffs;
    uint8_t *best_move, *status;
    u32 *nodes, *ran;
    u64* root_boards;
    uint8_t* root_turn;
    Trees t;
};

template <bool kIterate>
__global__ __launch_bounds__(kBlock) void tree_walk_kernel(SearchArgs a) {
    __shared__ u64 rays[kIterate ? kTabRows * 64 : 1];
    __shared__ uint8_t kth_tab[kIterate ? 256 * 8 : 1];
    __shared__ u32 path[kIterate ? OTHU_PATH_ENTRIES : 1];
    static_assert(!kIterate || sizeof(rays) + sizeof(kth_tab) + sizeof(path) == OTHR_LDS_BYTES,
                  "the header's LDS figure");
    if (kIterate) {
        kth_table_init(kth_tab);
        ray_table_init(rays);
        __syncthreads();
    }
    const u32 lane = threadIdx.x;
    Wave wave{lane, path, rays, kth_tab};

    for (u64 i = blockIdx.x; i < a.t.n; i += gridDim.x) {  // (uniform in the block)
        const Record r = a.t.records[i];
        const bool ok = a.t.ready(r);
        u32 n = 0, s = 0, nodes = 0, root_n = 0, root_s = 0, best = OTHU_NO_MOVE, ran = 0;
        int d = 0, root_d = 0;
        u64 P = 0, O = 0;
        if (ok) {
            SlabTree tree = a.t.tree(i);
            nodes = r.nodes;
            if (kIterate) {
                const u32 want = a.per_tree ? a.per_tree[i] : a.iterations;
                const u32 seen = tree.n(0u);
                const u32 room = seen < othu::kMaxIterations ? othu::kMaxIterations - seen : 0u;
                ran = want < room ? want : room;
                if (ran) {
                    nodes = othu::iterate<MctsRules>(tree, wave, r.id_base, r.played, ran, r.nodes,
                                                     othu::kMaxIterations, a.p);  // (ends in a sync)
                    if (lane == 0) {
                        a.t.records[i].played = r.played + ran;
                        a.t.records[i].nodes = nodes;
                    }
                }
            }
            tree.pos(0u, P, O);
            best = othud::root_rows(tree, P, O, lane, n, s, d);
            tree.visits_wins(0u, root_n, root_s);
            root_d = tree.d(0u);
        }
        if (a.visits) a.visits[i * 64 + lane] = n;
        if (a.wins) a.wins[i * 64 + lane] = s;
        if (a.diffs) a.diffs[i * 64 + lane] = d;
        if (lane == 0) {
            const bool white = r.turn == OTH_WHITE;
            if (a.root_wins) a.root_wins[i] = ok ? 128u * root_n - root_s : 0u;
            if (a.root_diffs) a.root_diffs[i] = -root_d;
            if (a.best_move) a.best_move[i] = (uint8_t)best;
            if (a.status) a.status[i] = ok ? OTHR_READY : OTHR_INVALID;
            if (a.nodes) a.nodes[i] = nodes;
            if (a.ran) a.ran[i] = ran;
            if (a.root_boards) {
                a.root_boards[2 * i] = white ? O : P;
                a.root_boards[2 * i + 1] = white ? P : O;
            }
            if (a.root_turn) a.root_turn[i] = white ? OTH_WHITE : OTH_BLACK;
        }
    }
}

// ---- advance ----
// the wave of the advance: lane k is node k of a turn's queue, and child k of a block
struct ScanWave {
    u32 lane_, word_, below_;
    template <class F>
    __device__ __forceinline__ void each(u32 count, F f) const {
        for (u32 k = lane_; k < count; k += othu::kLanes) f(k);
    }
    template <class F>
    __device__ __forceinline__ u32 scan(u32 count, F f) {
        u32 word = 0, weight = 0;
        if (lane_ < count) f(lane_, word, weight);
        u32 sum = weight;  // inclusive
#pragma unroll
        for (int d = 1; d < (int)othu::kLanes; d <<= 1) {
            const u32 below = (u32)__shfl_up((int)sum, d);
            if (lane_ >= (u32)d) sum += below;
        }
        word_ = word;
        below_ = sum - weight;
        return (u32)__builtin_amdgcn_readfirstlane(__shfl((int)sum, (int)othu::kLanes - 1));
    }
    __device__ __forceinline__ u32 scan_word(u32 k) const {
        return (u32)__builtin_amdgcn_readfirstlane(__shfl((int)word_, (int)k));
    }
    __device__ __forceinline__ u32 scan_below(u32 k) const {
        return (u32)__builtin_amdgcn_readfirstlane(__shfl((int)below_, (int)k));
    }
};

struct AdvanceArgs {
    const uint8_t* move;
    u32 keep;
    uint8_t* status;
    Trees t;
};

__global__ __launch_bounds__(kBlock) void tree_advance_kernel(AdvanceArgs a) {
    ScanWave wave{threadIdx.x, 0u, 0u};
    for (u64 i = blockIdx.x; i < a.t.n; i += gridDim.x) {  // (uniform in the block)
        const Record r = a.t.records[i];
        const u32 move = a.move[i];
        u32 st = a.t.ready(r) ? OTHR_READY : OTHR_INVALID;
        if (st == OTHR_READY && move != OTHR_KEEP) {
            SlabTree tree = a.t.tree(i), half = a.t.half(i);
            u64 P, O;
            tree.pos(0u, P, O);
            if (!othu::may_play<MctsRules>(P, O, move)) {
                st = OTHR_BADMOVE;
            } else {
                const u32 nodes = othu::advance<MctsRules>(tree, half, wave, move, a.keep != 0u, a.t.max_nodes);
                if (wave.lane_ == 0) {
                    a.t.records[i].nodes = nodes;
                    a.t.records[i].turn = r.turn == OTH_WHITE ? OTH_BLACK : OTH_WHITE;
                }
            }
        }
        if (wave.lane_ == 0 && a.status) a.status[i] = (uint8_t)st;
    }
}

othd::ResidentBlocks g_search_resident, g_rows_resident, g_advance_resident;

int64_t capped(int64_t n) { return n > (int64_t)OTHU_MAX_BLOCKS ? (int64_t)OTHU_MAX_BLOCKS * kBlock : n * kBlock; }

int search_grid(int64_t n) {
    return othd::launch_grid(g_search_resident, reinterpret_cast<const void*>(tree_walk_kernel<true>), kBlock,
                             capped(n), "OTH_MCTS_BLOCKS");
}
int rows_grid(int64_t n) {
    return othd::launch_grid(g_rows_resident, reinterpret_cast<const void*>(tree_walk_kernel<false>), kBlock,
                             capped(n), "OTH_MCTS_BLOCKS");
}
int advance_grid(int64_t n) {
    return othd::launch_grid(g_advance_resident, reinterpret_cast<const void*>(tree_advance_kernel), kBlock, capped(n),
                             "OTH_MCTS_BLOCKS");
}

// OTH_OK with `t` filled in, or the answer of a call that may not launch
int trees_of(int max_nodes, void* slabs, int64_t slab_bytes, void* records, int64_t record_bytes, int64_t n, Trees& t) {
    if (n < 0 || max_nodes < 1 || max_nodes > OTHU_MAX_NODES) return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    if (!slabs || ((uintptr_t)slabs & 15) || slab_bytes < othr_trees_slab_bytes(n, max_nodes) || !records ||
        ((uintptr_t)records & 7) || record_bytes < othr_trees_record_bytes(n))
        return OTH_EINVAL;
    t.slabs = static_cast<char*>(slabs);
    t.records = static_cast<Record*>(records);
    t.max_nodes = (u32)max_nodes;
    t.n = (u64)n;
    return OTH_OK;
}

template <bool kIterate>
int walk(SearchArgs& a, int64_t n, void* stream) {
    const int grid = kIterate ? search_grid(n) : rows_grid(n);
    if (grid <= 0) return status_of(hipErrorInvalidDevice);
    tree_walk_kernel<kIterate><<<(unsigned)grid, kBlock, 0, (hipStream_t)stream>>>(a);
    return status_of(hipGetLastError());
}

}  // namespace

extern "C" {

int64_t othr_trees_slab_bytes(int64_t n, int max_nodes) {
    if (n < 0 || max_nodes < 1 || max_nodes > OTHU_MAX_NODES) return OTH_EINVAL;
    return std::max<int64_t>(n * 2 * (int64_t)max_nodes * OTHU_NODE_BYTES, 16);
}

int64_t othr_trees_record_bytes(int64_t n) {
    if (n < 0) return OTH_EINVAL;
    return std::max<int64_t>(n * OTHR_RECORD_BYTES, 16);
}

int othr_trees_grid(int64_t n) {
    return othd::grid_answer(n, [n] { return search_grid(n); });
}

int othr_init(const uint64_t* boards, const uint8_t* turn, const uint64_t* id_base, uint64_t game_id0, uint64_t stride,
              int max_nodes, void* slabs, int64_t slab_bytes, void* records, int64_t record_bytes, int64_t n,
              void* stream) {
    InitArgs a;
    const int rc = trees_of(max_nodes, slabs, slab_bytes, records, record_bytes, n, a.t);
    if (rc != OTH_OK || n == 0) return rc;
    if (!boards) return OTH_EINVAL;
    a.boards = boards;
    a.turn = turn;
    a.id_base = id_base;
    a.game_id0 = game_id0;
    a.stride = stride;
    tree_init_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(a);
    return status_of(hipGetLastError());
}

int othr_search(int iterations, const uint32_t* iterations_per_tree, float explore, const float* log_table,
                uint64_t seed, int max_nodes, uint32_t* visits, uint32_t* wins, int32_t* diffs, uint32_t* root_wins,
                int32_t* root_diffs, uint8_t* best_move, uint8_t* status, uint32_t* nodes, uint32_t* ran,
                uint64_t* root_boards, uint8_t* root_turn, void* slabs, int64_t slab_bytes, void* records,
                int64_t record_bytes, int64_t n, void* stream) {
    if (iterations < 0 || iterations > OTHU_MAX_ITERATIONS || !log_table) return OTH_EINVAL;
    SearchArgs a;
    const int rc = trees_of(max_nodes, slabs, slab_bytes, records, record_bytes, n, a.t);
    if (rc != OTH_OK || n == 0) return rc;
    a.iterations = (u32)iterations;
    a.per_tree = iterations_per_tree;
    a.p.iterations = 0;
    a.p.max_nodes = (u32)max_nodes;
    a.p.explore = explore;
    a.p.log_table = log_table;
    a.p.seed_state = othp::seed_state(seed);
    a.p.game_id0 = 0;
    a.visits = visits;
    a.wins = wins;
    a.diffs = diffs;
    a.root_wins = root_wins;
    a.root_diffs = root_diffs;
    a.best_move = best_move;
    a.status = status;
    a.nodes = nodes;
    a.ran = ran;
    a.root_boards = root_boards;
    a.root_turn = root_turn;
    return walk<true>(a, n, stream);
}

int othr_rows(int max_nodes, uint32_t* visits, uint32_t* wins, int32_t* diffs, uint32_t* root_wins, int32_t* root_diffs,
              uint8_t* best_move, uint8_t* status, uint32_t* nodes, uint32_t* ran, uint64_t* root_boards,
              uint8_t* root_turn, void* slabs, int64_t slab_bytes, void* records, int64_t record_bytes, int64_t n,
              void* stream) {
    SearchArgs a;
    const int rc = trees_of(max_nodes, slabs, slab_bytes, records, record_bytes, n, a.t);
    if (rc != OTH_OK || n == 0) return rc;
    a.iterations = 0;
    a.per_tree = nullptr;
    a.p = othu::Params{};
    a.visits = visits;
    a.wins = wins;
    a.diffs = diffs;
    a.root_wins = root_wins;
    a.root_diffs = root_diffs;
    a.best_move = best_move;
    a.status = status;
    a.nodes = nodes;
    a.ran = ran;
    a.root_boards = root_boards;
    a.root_turn = root_turn;
    return walk<false>(a, n, stream);
}

int othr_advance(const uint8_t* move, int keep, int max_nodes, uint8_t* status, void* slabs, int64_t slab_bytes,
                 void* records, int64_t record_bytes, int64_t n, void* stream) {
    AdvanceArgs a;
    const int rc = trees_of(max_nodes, slabs, slab_bytes, records, record_bytes, n, a.t);
    if (rc != OTH_OK || n == 0) return rc;
    if (!move) return OTH_EINVAL;
    a.move = move;
    a.keep = keep != 0;
    a.status = status;
    const int grid = advance_grid(n);
    if (grid <= 0) return status_of(hipErrorInvalidDevice);
    tree_advance_kernel<<<(unsigned)grid, kBlock, 0, (hipStream_t)stream>>>(a);
    return status_of(hipGetLastError());
}

}  // extern "C"
