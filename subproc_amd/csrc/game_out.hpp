// game_out.hpp — what a game kernel (play.hip's, budget.hip's) writes for a
// game, stated once: its move record and its outputs.  Both are force-inlined
// into the kernels' loops; emit() reads the output pointers of the kernel's own
// argument struct (PlayArgs, BudgetPlayArgs: same names, layouts of their own).
#pragma once
#include "../../include/othello.h"
#include "play_core.hpp"

namespace othp {

// a game's move record: the row starts 255-padded, a move is one byte store
struct MoveRecord {
    uint8_t* row;  // NULL: no record
    __device__ __forceinline__ void pad() const {
        if (!row) return;
#pragma unroll
        for (int q = 0; q < OTH_MOVES_STRIDE / 16; q++) reinterpret_cast<uint4*>(row)[q] = make_uint4(~0u, ~0u, ~0u, ~0u);
    }
    __device__ __forceinline__ void move(othm::u32 ply, othm::u32 code) const {
        if (row && ply < (othm::u32)OTH_MOVES_STRIDE) row[ply] = (uint8_t)code;
    }
};

// game g has ended (G.status says how): its outputs, and the histogram's bins
// if it was played to its end
template <class Args>
__device__ __forceinline__ void emit(const Args& a, othm::u64 g, const Game& G) {
    const othm::u64 bl = black_of(G), wh = white_of(G);
    const int d = G.status == othm::kInvalid ? 0 : __popcll(bl) - __popcll(wh);
    if (a.a_black) a.a_black[g] = (uint8_t)G.a_black;
    if (a.final_boards) reinterpret_cast<ulonglong2*>(a.final_boards)[g] = make_ulonglong2(bl, wh);
    if (a.diff) a.diff[g] = (int8_t)d;
    if (a.plies) a.plies[g] = (uint8_t)G.ply;
    if (a.status) a.status[g] = (uint8_t)G.status;
    if (a.nodes) a.nodes[g] = G.nodes;
    if (a.hist && G.status == othm::kSearched) {
        atomicAdd(&a.hist[d + 64], 1ull);
        atomicAdd(&a.hist[d > 0 ? 129 : (d < 0 ? 130 : 131)], 1ull);
        atomicAdd(&a.hist[132], (unsigned long long)G.ply);
    }
}

}  // namespace othp
