// mcts_wide.hip — the wide Monte Carlo tree search for gfx950
// (include/othello_mcts_wide.h): mcts.hip's search with L leaves
// per iteration, one block of L waves per tree.
//
// One kernel.  A block is L waves and stays persistent over its trees: block b
// searches positions b, b + grid, ... and keeps the tree it is at in slab b of
// the caller's scratch (mcts_device.hpp's SlabTree).  mcts_wide_core.hpp's
// search_wide() is the walk.  Wave 0 selects, expands and marks for the L
// walkers one after another, leaving each walker's path and leaf in LDS, while
// the other waves wait at the block's barrier; then wave w plays walker w's 64
// games (Wave::playout) and adds their sums along its path with vector atomics
// that return nothing.  A round has two barriers, each a release/acquire fence
// at workgroup scope around s_barrier: the waves of a block share a compute
// unit and its L1, so nothing is ordered at agent scope.  No wave spins on
// memory, no block reads another block's slab.
// The finish (the rows, the root's sums, the best move) is the tail of the same
// kernel: lane sq of wave 0 writes square sq.
#include "../../include/othello_mcts_wide.h"
#include "mcts_device.hpp"
#include "mcts_wide_core.hpp"

static_assert(OTHV_MAX_LEAVES == othu::kMaxLeaves, "the header's constant is the core's");

namespace {

using namespace oth;
using othd::status_of;
using othud::MctsRules;
using othud::SlabTree;
using othud::Wave;

constexpr int kWave = othud::kBlock;
constexpr int kMaxBlock = kWave * OTHV_MAX_LEAVES;

// the block: the calling wave (mcts_device.hpp's Wave) and the walkers' paths and leaves in LDS
struct Block : Wave {
    u32 wave_id;        // uniform in the wave
    u32* paths;         // LDS [OTHV_MAX_LEAVES][OTHU_PATH_ENTRIES]
    ulonglong2* leaves; // LDS [OTHV_MAX_LEAVES] the leaf's (P to move, O)
    u32* depths;        // LDS [OTHV_MAX_LEAVES] the leaf's place in its path

    template <class F>
    __device__ __forceinline__ void walkers(u32 count, F f) const {
        if (wave_id == 0)
            for (u32 w = 0; w < count; w++) f(w);
    }
    template <class F>
    __device__ __forceinline__ void waves(u32 count, F f) const {
        if (wave_id < count) f(wave_id);
    }
    // a phase's writes (slab and LDS) by one wave before the next phase's reads by another wave of this block
    // (the explicit wait after the fence, as in SlabTree::sync(): the stores and atomics are complete)
    __device__ __forceinline__ void barrier() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    using Wave::sync;
    __device__ __forceinline__ void path_set(u32 w, u32 k, u32 v) const {
        if (lane_ == 0 && k < othu::kPathEntries) paths[w * othu::kPathEntries + k] = v;
    }
    __device__ __forceinline__ u32 path_get(u32 w, u32 k) const {
        return paths[w * othu::kPathEntries + (k < othu::kPathEntries ? k : 0u)];
    }
    __device__ __forceinline__ void leaf_set(u32 w, u64 P, u64 O, u32 depth) const {
        if (lane_ == 0) {
            leaves[w] = make_ulonglong2(P, O);
            depths[w] = depth;
        }
    }
    __device__ __forceinline__ void leaf_get(u32 w, u64& P, u64& O, u32& depth) const {
        const ulonglong2 b = leaves[w];
        P = b.x;
        O = b.y;
        const u32 d = depths[w];
        depth = d < othu::kPathEntries ? d : 0u;  // (never: a lane's index into the path stays inside it)
    }
};

struct Args {
    const u64* boards;
    const uint8_t* turn;
    othu::Params p;
    u32 leaves;
    u32 *visits, *wins;
    int* diffs;
    u32* root_wins;
    int* root_diffs;
    uint8_t *best_move, *status;
    u32* nodes;
    char* scratch;
    u64 n;
};

__global__ __launch_bounds__(kMaxBlock) void mcts_wide_rounds(Args a) {
    __shared__ u64 rays[kTabRows * 64];
    __shared__ uint8_t kth_tab[256 * 8];
    __shared__ u32 paths[OTHV_MAX_LEAVES * OTHU_PATH_ENTRIES];
    __shared__ ulonglong2 leaves[OTHV_MAX_LEAVES];
    __shared__ u32 depths[OTHV_MAX_LEAVES];
    static_assert(sizeof(rays) + sizeof(kth_tab) + sizeof(paths) + sizeof(leaves) + sizeof(depths) == OTHV_LDS_BYTES,
                  "the header's LDS figure");
    kth_table_init(kth_tab);
    ray_table_init(rays);
    __syncthreads();

    const u32 lane = threadIdx.x & (kWave - 1);
    const u32 wave_id = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const u64 M = a.p.max_nodes;
    char* slab = a.scratch + (u64)blockIdx.x * M * OTHU_NODE_BYTES;
    SlabTree tree = othud::slab_tree(slab, M);
    Block block{{lane, paths, rays, kth_tab}, wave_id, paths, leaves, depths};

    for (u64 i = blockIdx.x; i < a.n; i += gridDim.x) {  // (uniform in the block)
        const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.boards)[i];
        const bool white = a.turn && a.turn[i] == OTH_WHITE;
        const u64 P = white ? b.y : b.x, O = white ? b.x : b.y;
        const bool valid = (b.x & b.y) == 0;
        u32 n = 0, s = 0, nodes = 0, root_n = 0, root_s = 0, best = OTHU_NO_MOVE;
        int d = 0, root_d = 0;
        if (valid) nodes = othu::search_wide<MctsRules>(tree, block, P, O, i, a.leaves, a.p);  // (ends in a barrier)
        if (wave_id != 0) continue;  // the other waves touch no slab before the next tree's first barrier
        if (valid) {
            best = othud::root_rows(tree, P, O, lane, n, s, d);
            tree.visits_wins(0u, root_n, root_s);
            root_d = tree.d(0u);
            tree.sync();  // the rows are read before the next tree overwrites the slab
        }
        if (a.visits) a.visits[i * 64 + lane] = n;
        if (a.wins) a.wins[i * 64 + lane] = s;
        if (a.diffs) a.diffs[i * 64 + lane] = d;
        if (lane == 0) {
            if (a.root_wins) a.root_wins[i] = valid ? 128u * root_n - root_s : 0u;
            if (a.root_diffs) a.root_diffs[i] = -root_d;
            if (a.best_move) a.best_move[i] = (uint8_t)best;
            if (a.status) a.status[i] = valid ? OTHU_SEARCHED : OTHU_INVALID;
            if (a.nodes) a.nodes[i] = nodes;
        }
    }
}

othd::ResidentBlocks g_resident[OTHV_MAX_LEAVES + 1];  // by L: the block's size decides how many a CU holds

bool leaves_ok(int leaves) { return leaves >= 1 && leaves <= OTHV_MAX_LEAVES; }

int wide_grid(int64_t n, int leaves) {
    const int block = kWave * leaves;
    const int g = othd::launch_grid(g_resident[leaves], reinterpret_cast<const void*>(mcts_wide_rounds), block,
                                    std::min<int64_t>(n, OTHV_MAX_BLOCKS) * block, "OTH_MCTS_WIDE_BLOCKS");
    return std::min(g, (int)OTHV_MAX_BLOCKS);
}

int64_t slabs_for(int64_t n) { return std::min<int64_t>(n, OTHV_MAX_BLOCKS); }

}  // namespace

extern "C" {

int64_t othv_mcts_wide_scratch_bytes(int64_t n, int max_nodes, int leaves) {
    if (n < 0 || max_nodes < 1 || max_nodes > OTHU_MAX_NODES || !leaves_ok(leaves)) return OTH_EINVAL;
    return std::max<int64_t>(slabs_for(n) * (int64_t)max_nodes * OTHU_NODE_BYTES, 16);
}

int othv_mcts_wide_grid(int64_t n, int leaves) {
    if (!leaves_ok(leaves)) return OTH_EINVAL;
    return othd::grid_answer(n, [n, leaves] { return wide_grid(n, leaves); });
}

int othv_mcts_wide(const uint64_t* boards, const uint8_t* turn, int iterations, int leaves, float explore,
                   const float* log_table, uint64_t seed, uint64_t game_id0, int max_nodes, uint32_t* visits,
                   uint32_t* wins, int32_t* diffs, uint32_t* root_wins, int32_t* root_diffs, uint8_t* best_move,
                   uint8_t* status, uint32_t* nodes, void* scratch, int64_t scratch_bytes, int64_t n, void* stream) {
    if (n < 0 || !leaves_ok(leaves) || iterations < 1 || (int64_t)iterations * leaves > OTHU_MAX_ITERATIONS ||
        max_nodes < 1 || max_nodes > OTHU_MAX_NODES || !log_table)
        return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    if (!boards || !scratch || ((uintptr_t)scratch & 15) ||
        scratch_bytes < othv_mcts_wide_scratch_bytes(n, max_nodes, leaves))
        return OTH_EINVAL;
    const int grid = wide_grid(n, leaves);  // <= min(n, OTHV_MAX_BLOCKS): a slab per block
    if (grid <= 0) return status_of(hipErrorInvalidDevice);
    Args a;
    a.boards = boards;
    a.turn = turn;
    a.p.iterations = (u32)iterations;
    a.p.max_nodes = (u32)max_nodes;
    a.p.explore = explore;
    a.p.log_table = log_table;
    a.p.seed_state = othp::seed_state(seed);
    a.p.game_id0 = game_id0;
    a.leaves = (u32)leaves;
    a.visits = visits;
    a.wins = wins;
    a.diffs = diffs;
    a.root_wins = root_wins;
    a.root_diffs = root_diffs;
    a.best_move = best_move;
    a.status = status;
    a.nodes = nodes;
    a.scratch = static_cast<char*>(scratch);
    a.n = (u64)n;
    mcts_wide_rounds<<<(unsigned)grid, (unsigned)(kWave * leaves), 0, (hipStream_t)stream>>>(a);
    return status_of(hipGetLastError());
}

}  // extern "C"
