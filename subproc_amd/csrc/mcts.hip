// mcts.hip — Monte Carlo tree search for gfx950 (include/othello_mcts.h,
// DESIGN.md §28): UCT over uniform random playouts, one wave per tree.
//
// One kernel.  A block is one wave, as in search.hip, and stays persistent over
// its trees: block b searches positions b, b + grid, ... and keeps the tree it
// is at in slab b of the caller's scratch.  mcts_core.hpp's search() is the
// walk; mcts_device.hpp gives it the tree's memory (SlabTree), the wave (Wave)
// and the playout, shared with mcts_tree.hip.
// The finish (the rows, the root's sums, the best move) is the tail of the same
// kernel: lane sq writes square sq.
#include "mcts_device.hpp"

namespace {

using namespace oth;
using othd::status_of;
using othud::kBlock;
using othud::MctsRules;
using othud::SlabTree;
using othud::Wave;

struct Args {
    const u64* boards;
    const uint8_t* turn;
    othu::Params p;
    u32 *visits, *wins;
    int* diffs;
    u32* root_wins;
    int* root_diffs;
    uint8_t *best_move, *status;
    u32* nodes;
    char* scratch;
    u64 n;
};

__global__ __launch_bounds__(kBlock) void mcts_kernel(Args a) {
    __shared__ u64 rays[kTabRows * 64];
    __shared__ uint8_t kth_tab[256 * 8];
    __shared__ u32 path[OTHU_PATH_ENTRIES];
    static_assert(sizeof(rays) + sizeof(kth_tab) + sizeof(path) == OTHU_LDS_BYTES, "the header's LDS figure");
    kth_table_init(kth_tab);
    ray_table_init(rays);
    __syncthreads();

    const u32 lane = threadIdx.x;
    const u64 M = a.p.max_nodes;
    char* slab = a.scratch + (u64)blockIdx.x * M * OTHU_NODE_BYTES;
    SlabTree tree = othud::slab_tree(slab, M);
    Wave wave{lane, path, rays, kth_tab};

    for (u64 i = blockIdx.x; i < a.n; i += gridDim.x) {  // (uniform in the block)
        const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.boards)[i];
        const bool white = a.turn && a.turn[i] == OTH_WHITE;
        const u64 P = white ? b.y : b.x, O = white ? b.x : b.y;
        const bool valid = (b.x & b.y) == 0;
        u32 n = 0, s = 0, nodes = 0, root_n = 0, root_s = 0, best = OTHU_NO_MOVE;
        int d = 0, root_d = 0;
        if (valid) {
            nodes = othu::search<MctsRules>(tree, wave, P, O, i, a.p);  // (ends in a sync)
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

othd::ResidentBlocks g_resident;

int mcts_grid(int64_t n) {
    const int g = othd::launch_grid(g_resident, reinterpret_cast<const void*>(mcts_kernel), kBlock,
                                    n > (int64_t)OTHU_MAX_BLOCKS ? (int64_t)OTHU_MAX_BLOCKS * kBlock : n * kBlock,
                                    "OTH_MCTS_BLOCKS");
    return g;
}

int64_t slabs_for(int64_t n) { return std::min<int64_t>(n, OTHU_MAX_BLOCKS); }

}  // namespace

extern "C" {

int64_t othu_mcts_scratch_bytes(int64_t n, int max_nodes) {
    if (n < 0 || max_nodes < 1 || max_nodes > OTHU_MAX_NODES) return OTH_EINVAL;
    return std::max<int64_t>(slabs_for(n) * (int64_t)max_nodes * OTHU_NODE_BYTES, 16);
}

int othu_mcts_grid(int64_t n) {
    return othd::grid_answer(n, [n] { return mcts_grid(n); });
}

int othu_mcts(const uint64_t* boards, const uint8_t* turn, int iterations, float explore, const float* log_table,
              uint64_t seed, uint64_t game_id0, int max_nodes, uint32_t* visits, uint32_t* wins, int32_t* diffs,
              uint32_t* root_wins, int32_t* root_diffs, uint8_t* best_move, uint8_t* status, uint32_t* nodes,
              void* scratch, int64_t scratch_bytes, int64_t n, void* stream) {
    if (n < 0 || iterations < 1 || iterations > OTHU_MAX_ITERATIONS || max_nodes < 1 || max_nodes > OTHU_MAX_NODES ||
        !log_table)
        return OTH_EINVAL;
    if (n == 0) return OTH_OK;
    if (!boards || !scratch || ((uintptr_t)scratch & 15) || scratch_bytes < othu_mcts_scratch_bytes(n, max_nodes))
        return OTH_EINVAL;
    const int grid = mcts_grid(n);  // <= min(n, OTHU_MAX_BLOCKS): a slab per block
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
    mcts_kernel<<<(unsigned)grid, kBlock, 0, (hipStream_t)stream>>>(a);
    return status_of(hipGetLastError());
}

}  // extern "C"
