// mcts_device.hpp — what the kernels of the Monte Carlo tree searches share
// (mcts.hip: a tree per call; mcts_tree.hip: trees that persist): the rules,
// the tree's memory in a slab of OTHU_NODE_BYTES a node, and the wave with its
// playout.  mcts_core.hpp's walk is written over these.
//   * SlabTree: three arrays per slab, the boards (16 B a node), (n, s) and
//     (d, children) (8 B each), so that the children of a node are one
//     coalesced access in selection.  Words written by one lane are read by
//     another lane of the same wave in the next phase: sync() is a
//     release/acquire fence at workgroup scope and a wave barrier.  No wave
//     reads another wave's slab, so nothing is ordered at agent scope, nothing
//     is atomic and nothing waits;
//   * Wave: lane k is child k in selection (a ballot for the first unvisited
//     child, an argmax by shuffles otherwise) and in expansion, path node k in
//     the back-up (the path lives in LDS), and playout k of the iteration;
//   * the playout: othello.hip's random ply, two plies per turn of the loop
//     with no register swap (analyse<789>, kth_bit_off, flips_col, place over
//     the ray and k-th bit tables in LDS), all 64 lanes from the same leaf in
//     lockstep until the last game ends.  W and D are ballots, popcounts and a
//     shuffle sum.
// Everything is force-inlined: no kernel gets a symbol from here.
#pragma once
#include "../../include/othello_mcts.h"
#include "device_common.hpp"
#include "mcts_core.hpp"
#include "play_core.hpp"  // DESIGN.md §4's draws: seed_state, game_key, Rng

static_assert(OTHU_MAX_ITERATIONS == othu::kMaxIterations && OTHU_MAX_NODES == othu::kMaxNodes &&
                  OTHU_PATH_ENTRIES == othu::kPathEntries && OTHU_SEARCHED == othu::kSearched &&
                  OTHU_INVALID == othu::kInvalid && OTHU_NO_MOVE == othu::kNoMove && OTH_PASS == othu::kPassMove,
              "the header's constants are the core's");

namespace othud {

using namespace oth;

constexpr int kBlock = 64;  // one wave
static_assert(kBlock == (int)othu::kLanes, "a lane per playout");

struct MctsRules : othd::DeviceRules {
    static __device__ __forceinline__ u32 kth(u64 m, u32 k) { return kth_bit(m, k); }
};

// ---- the tree's memory: one slab ----
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
    // the wide search's two halves of add_stats (mcts_wide_core.hpp): the visit by the one wave that selects; the
    // sums by any wave of the block, as vector atomics that return nothing (integer adds: any order, the same words)
    __device__ __forceinline__ void mark(u32 v) { ns[v].x += 1u; }
    __device__ __forceinline__ void add_result(u32 v, u32 s, int d) {
        __hip_atomic_fetch_add(&ns[v].y, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&dl[v].x, (u32)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // a phase's writes, made by one lane, before the next phase's reads by another lane of this wave
    // (the explicit wait after the fence: the stores are complete, not only ordered, before the wave goes on)
    __device__ __forceinline__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }
};

// the tree in a slab of M nodes at `slab`
__device__ __forceinline__ SlabTree slab_tree(char* slab, u64 M) {
    return SlabTree{reinterpret_cast<ulonglong2*>(slab), reinterpret_cast<uint2*>(slab + kPosBytes * M),
                    reinterpret_cast<uint2*>(slab + (kPosBytes + kStatBytes) * M)};
}

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

// the rows of a tree at square `lane` and the root's best move (uniform), for
// the root (P to move, O): the tail of every kernel that answers a search
__device__ __forceinline__ u32 root_rows(SlabTree& tree, u64 P, u64 O, u32 lane, u32& n, u32& s, int& d) {
    const u64 legal = MctsRules::moves(P, O);
    u64 key = othu::root_entry<MctsRules>(tree, legal, lane, n, s, d);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        const u64 other = (u64)__shfl_xor((unsigned long long)key, k);
        key = other > key ? other : key;
    }
    return othu::best_move_of<MctsRules>(key, P, O);
}

}  // namespace othud
