// mcts.hip — Monte Carlo tree search for gfx950 (include/othello_mcts.h,
// DESIGN.md §28): UCT over uniform random playouts, one wave per tree.
//
// One kernel.  A block is one wave, as in search.hip, and stays persistent over
// its trees: block b searches positions b, b + grid, ... and keeps the tree it
// is at in slab b of the caller's scratch.  mcts_core.hpp's search() is the
// walk; this file gives it
//   * the tree's memory (SlabTree): three arrays per slab, the boards (16 B a
//     node), (n, s) and (d, children) (8 B each), so that the children of a
//     node are one coalesced access in selection.  Words written by one lane
//     are read by another lane of the same wave in the next phase: sync() is a
//     release/acquire fence at workgroup scope and a wave barrier.  No wave
//     reads another wave's slab, so nothing is ordered at agent scope, nothing
//     is atomic and nothing waits;
//   * the wave (Wave): lane k is child k in selection (a ballot for the first
//     unvisited child, an argmax by shuffles otherwise) and in expansion, path
//     node k in the back-up (the path lives in LDS), and playout k of the
//     iteration;
//   * the playout: othello.hip's random ply, two plies per turn of the loop
//     with no register swap (analyse<789>, kth_bit_off, flips_col, place over
//     the ray and k-th bit tables in LDS), all 64 lanes from the same leaf in
//     lockstep until the last game ends.  W and D are ballots, popcounts and a
//     shuffle sum.
// The finish (the rows, the root's sums, the best move) is the tail of the same
// kernel: lane sq writes square sq.
#include "../../include/othello_mcts.h"
#include "device_common.hpp"
#include "mcts_core.hpp"
#include "play_core.hpp"  // DESIGN.md §4's draws: seed_state, game_key, Rng

static_assert(OTHU_MAX_ITERATIONS == othu::kMaxIterations && OTHU_MAX_NODES == othu::kMaxNodes &&
                  OTHU_PATH_ENTRIES == othu::kPathEntries && OTHU_SEARCHED == othu::kSearched &&
                  OTHU_INVALID == othu::kInvalid && OTHU_NO_MOVE == othu::kNoMove && OTH_PASS == othu::kPassMove,
              "the header's constants are the core's");

namespace {

using namespace oth;
using othd::status_of;

constexpr int kBlock = 64;  // one wave
static_assert(kBlock == (int)othu::kLanes, "a lane per playout");

struct MctsRules : othd::DeviceRules {
    static __device__ __forceinline__ u32 kth(u64 m, u32 k) { return kth_bit(m, k); }
};

// ---- the tree's memory: slab b of scratch ----
constexpr int64_t kPosBytes = 16, kStatBytes = 8;
static_assert(kPosBytes + 2 * kStatBytes == OTHU_NODE_BYTES, "the header's node");

struct SlabTree {
    ulonglong2* posv;  // [M] the mover's discs, the other side's
    uint2* ns;         // [M] visits, half-points
    uint2* dl;         // [M] disc sum, children
    __device__ __forceinline__ void pos(u32 v, u64& P, u64& O) const {
        const ulonglong2 b = posv[v];
        P = b.x;
        O = b.y;
    }
    __device__ __forceinline__ void set_pos(u32 v, u64 P, u64 O) { posv[v] = make_ulonglong2(P, O); }
    __device__ __forceinline__ void visits_wins(u32 v, u32& n, u32& s) const {
        const uint2 w = ns[v];
        n = w.x;
        s = w.y;
    }
    __device__ __forceinline__ u32 n(u32 v) const { return ns[v].x; }
    __device__ __forceinline__ int d(u32 v) const { return (int)dl[v].x; }
    __device__ __forceinline__ u32 link(u32 v) const { return dl[v].y; }
    __device__ __forceinline__ void set_stats(u32 v, u32 n, u32 s, int d) {
        ns[v] = make_uint2(n, s);
        dl[v].x = (u32)d;
    }
    __device__ __forceinline__ void set_link(u32 v, u32 link) { dl[v].y = link; }
    __device__ __forceinline__ void add_stats(u32 v, u32 n, u32 s, int d) {
        const uint2 w = ns[v];
        ns[v] = make_uint2(w.x + n, w.y + s);
        dl[v].x += (u32)d;
    }
    // a phase's writes, made by one lane, before the next phase's reads by another lane of this wave
    // (the explicit wait after the fence: the stores are complete, not only ordered, before the wave goes on)
    __device__ __forceinline__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }
};

// ---- the wave ----
struct Wave {
    u32 lane_;
    u32* path;              // LDS [OTHU_PATH_ENTRIES]
    const u64* rays;        // LDS ray table
    const uint8_t* kth_tab; // LDS k-th bit table

    template <class F>
    __device__ __forceinline__ void each(u32 count, F f) const {
        for (u32 k = lane_; k < count; k += othu::kLanes) f(k);
    }
    // the first fresh child, else the best by othu::better(); cnt in 1..64
    template <class F>
    __device__ __forceinline__ u32 pick(u32 cnt, F f) const {
        bool fresh = false;
        float sc = -__builtin_inff();  // a lane without a child loses to every child (scores are >= 0)
        u32 idx = lane_;
        if (lane_ < cnt) f(lane_, fresh, sc);
        const u64 m = __ballot(fresh);
        if (m == 0) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const float so = __shfl_xor(sc, d);
                const u32 io = (u32)__shfl_xor((int)idx, d);
                if (othu::better(so, io, sc, idx)) {
                    sc = so;
                    idx = io;
                }
            }
        } else {
            idx = (u32)__builtin_ctzll(m);
        }
        // one value in every lane, and a child of this node whatever the table held
        idx = (u32)__builtin_amdgcn_readfirstlane((int)idx);
        return idx < cnt ? idx : cnt - 1u;
    }
    __device__ __forceinline__ void path_set(u32 k, u32 v) const {
        if (lane_ == 0 && k < othu::kPathEntries) path[k] = v;
    }
    __device__ __forceinline__ u32 path_get(u32 k) const { return path[k < othu::kPathEntries ? k : 0u]; }
    // the path: written by lane 0, read by lane k (a wave's LDS operations are in order)
    __device__ __forceinline__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }

    // the iteration's 64 games from (P to move, O): lane j plays id0 + j.  W, D
    // from the point of view of the opponent of the leaf's mover.
    __device__ __forceinline__ void playout(u64 P, u64 O, u64 id0, u64 seed_state, u32& W, int& D) const {
        othp::Rng rng;
        rng.init(othp::game_key(seed_state, id0 + (u64)lane_));
        bool passed = false;
        // one ply of mover X against Y; true at the terminal (othello.hip's ply_of
        // without the record and the ply count)
        auto ply_of = [&](u64& X, u64& Y) -> bool {
            Position pos;
            analyse<789>(X, Y, pos);
            const u64 legal = pos.legal;
            const u32 c_lo = __popc((u32)legal), nl = c_lo + __popc((u32)(legal >> 32));
            if (nl == 0) {
                if (passed || (X | Y) == ~0ull) return true;
                passed = true;
                return false;
            }
            passed = false;
            const u32 off = kth_bit_off(legal, rng.pick(nl), c_lo, kth_tab);
            const u64* col = ray_col(rays, off);
            const Flips f = flips_col(col[kRayRows * 64], run_sets(X, pos), col);
            place(X, Y, f);
            return false;
        };
        for (;;) {
            if (ply_of(P, O)) break;
            if (ply_of(O, P)) break;
        }
        const int dp = __popcll(O) - __popcll(P);
        W = 2u * (u32)__popcll(__ballot(dp > 0)) + (u32)__popcll(__ballot(dp == 0));
        int sum = dp;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
        D = sum;
    }
};

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
    SlabTree tree{reinterpret_cast<ulonglong2*>(slab), reinterpret_cast<uint2*>(slab + kPosBytes * M),
                  reinterpret_cast<uint2*>(slab + (kPosBytes + kStatBytes) * M)};
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
            const u64 legal = MctsRules::moves(P, O);
            u64 key = othu::root_entry<MctsRules>(tree, legal, lane, n, s, d);
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) {
                const u64 other = (u64)__shfl_xor((unsigned long long)key, k);
                key = other > key ? other : key;
            }
            best = othu::best_move_of<MctsRules>(key, P, O);
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
