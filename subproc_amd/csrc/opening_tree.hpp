// opening_tree.hpp — the per-device opening tree of the random rollout kernel.
//
// Every random game from the standard opening recomputes the same first plies:
// the analysis, the fills and the flips of ply d are functions of the path of
// picks alone.  The tree holds every position reachable from the opening in at
// most kOpeningDepthMax plies, indexed by that path and not merged by
// transposition, so a game finds its position after D plies from its D draws:
//     node = 0; D times: (child_base, nl) = nodes[node]; node = child_base + pick(nl)
// The walk is a chain of dependent reads whose latency the kernel does not
// hide: measured, every dependent read from memory costs the headline 3-4%,
// more than two computed plies.  So every block copies the
// upper part of the tree to LDS: the nodes of depth 0..min(D, 6) - 1 and, for
// D <= kOpeningLdsLeafDepth, the leaf level's boards as well, so that a walk
// of the shipped depth reads nothing from memory.  Deeper walks read the
// levels below 6 and their leaves from memory.
// The draws are the ones the ply loop makes (one per placement, pick(nl) with
// the same nl), so every later draw and every game is unchanged.
//
// Layout (one device allocation, < 8 MB): boards[455,221] as (mover's discs,
// opponent's discs), 16 B each, all levels; nodes[65,005] as one word each,
// child_base << 5 | nl (nl <= 31, checked by the build), levels 0..7; then the
// level counters and the error word of the build.  Indices are global: level
// d occupies [opening_off(d), opening_off(d + 1)).  A node's children lie
// consecutively in LSB-first order of its legal mask (the order kth_bit_off
// picks in); the order of nodes within a level is whatever the build's
// atomics made it, since only child_base is followed.
//
// No node of depth <= 7 is without a legal move (the build checks it), so a
// walk never meets a pass or a terminal; 24 of the depth-8 nodes have no move
// for the side to move and are leaves like the others.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bitboard.hpp"

namespace oth {

constexpr int kOpeningDepthMax = 8;
// positions by path at depth 0..8 (perft of the standard opening)
constexpr u32 kOpeningLevel[kOpeningDepthMax + 1] = {1, 4, 12, 56, 244, 1396, 8200, 55092, 390216};
constexpr u32 opening_off(int d) {
    u32 s = 0;
    for (int i = 0; i < d; i++) s += kOpeningLevel[i];
    return s;
}
constexpr u32 kOpeningInternal = opening_off(kOpeningDepthMax);   // 65,005 nodes of depth 0..7
constexpr u32 kOpeningNodes = opening_off(kOpeningDepthMax + 1);  // 455,221 positions
static_assert(kOpeningInternal == 65005u && kOpeningNodes == 455221u, "level sizes");
// build errors (the error word)
constexpr u32 kOpeningErrNoMove = 1u, kOpeningErrOverflow = 2u, kOpeningErrWide = 4u;
// a node word: child_base << kOpeningNlBits | nl
constexpr u32 kOpeningNlBits = 5u, kOpeningNlMask = (1u << kOpeningNlBits) - 1u;
static_assert(kOpeningNodes < (1u << (32u - kOpeningNlBits)), "child_base fits its field");
// the levels a block keeps in LDS: the nodes of depth 0..5 (1,713 words) at
// the most
constexpr int kOpeningLdsDepth = 6;
// up to this depth the leaf level's boards are kept in LDS as well (level 4:
// 244 boards, 3.9 KB), and a walk reads nothing from memory.  Level 5 (1,396
// boards, 22 KB) no longer fits beside a second launch's blocks: 6 blocks per
// CU of 17 KB static LDS each leave 9.6 KB per block.
constexpr int kOpeningLdsLeafDepth = 4;
// the dynamic LDS of a launch of this depth
constexpr size_t opening_lds_bytes(int depth) {
    return (depth > 0 && depth <= kOpeningLdsLeafDepth ? kOpeningLevel[depth] * sizeof(ulonglong2) : 0) +
           (depth > 0 ? opening_off(depth < kOpeningLdsDepth ? depth : kOpeningLdsDepth) * sizeof(u32) : 0);
}

struct OpeningTree {
    ulonglong2* boards;  // [kOpeningNodes]
    u32* nodes;          // [kOpeningInternal]: child_base << 5 | nl
    u32* count;          // [kOpeningDepthMax + 1] nodes placed per level, then the error word
};
constexpr size_t kOpeningBoardsBytes = (size_t)kOpeningNodes * sizeof(ulonglong2);
constexpr size_t kOpeningNodesBytes = (size_t)kOpeningInternal * sizeof(u32);
constexpr size_t kOpeningCountBytes = (kOpeningDepthMax + 2) * sizeof(u32);
constexpr size_t kOpeningBytes = kOpeningBoardsBytes + kOpeningNodesBytes + kOpeningCountBytes;
inline OpeningTree opening_tree_at(void* base) {
    char* p = static_cast<char*>(base);
    return OpeningTree{reinterpret_cast<ulonglong2*>(p), reinterpret_cast<u32*>(p + kOpeningBoardsBytes),
                       reinterpret_cast<u32*>(p + kOpeningBoardsBytes + kOpeningNodesBytes)};
}

__global__ void opening_root_kernel(OpeningTree t, u64 mover, u64 other) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        t.boards[0] = make_ulonglong2(mover, other);
        t.count[0] = 1u;
    }
}

// level d -> level d + 1: one thread per node of level d.  The node's children
// take nl consecutive slots of level d + 1 (one atomicAdd on that level's
// counter); child k is the position after the k-th legal square, seen from the
// side then to move.  off / off_next / end_next are the global indices of
// level d, of level d + 1 and of that level's end; a node without a move or
// with more moves than the node word holds, or children that would fall
// outside their level, set the error word and write nothing.
__global__ __launch_bounds__(256) void opening_level_kernel(OpeningTree t, int d, u32 off, u32 off_next, u32 end_next) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    // level d is complete (its kernel ran before on the stream), and never larger than its range
    if (i >= t.count[d] || i >= off_next - off) return;
    const ulonglong2 b = t.boards[off + i];
    const u64 P = b.x, O = b.y;
    u64 legal = moves(P, O);
    const u32 nl = (u32)__popcll(legal);
    if (nl == 0u || nl > kOpeningNlMask) {
        atomicOr(&t.count[kOpeningDepthMax + 1], nl ? kOpeningErrWide : kOpeningErrNoMove);
        return;
    }
    const u32 base = off_next + atomicAdd(&t.count[d + 1], nl);
    if (base < off_next || base > end_next || nl > end_next - base) {
        atomicOr(&t.count[kOpeningDepthMax + 1], kOpeningErrOverflow);
        return;
    }
    t.nodes[off + i] = base << kOpeningNlBits | nl;
    for (u32 k = 0; k < nl; k++) {
        const u32 sq = (u32)__ffsll((long long)legal) - 1u;
        legal &= legal - 1ull;
        const u64 f = flips_carry(sq, P, O);
        t.boards[base + k] = make_ulonglong2(O & ~f, P | f | (1ull << sq));
    }
}

// Builds the tree into `base` (kOpeningBytes of device memory) on stream s
// and waits for that stream only.  True when every level has its known size
// and no internal node lacks a move.
inline bool opening_tree_build(void* base, u64 open_mover, u64 open_other, hipStream_t s) {
    const OpeningTree t = opening_tree_at(base);
    if (hipMemsetAsync(t.count, 0, kOpeningCountBytes, s) != hipSuccess) return false;
    opening_root_kernel<<<1, 64, 0, s>>>(t, open_mover, open_other);
    for (int d = 0; d < kOpeningDepthMax; d++) {
        const u32 n = kOpeningLevel[d];
        opening_level_kernel<<<(n + 255u) / 256u, 256, 0, s>>>(t, d, opening_off(d), opening_off(d + 1),
                                                              opening_off(d + 2));
    }
    u32 count[kOpeningDepthMax + 2] = {};
    if (hipMemcpyAsync(count, t.count, kOpeningCountBytes, hipMemcpyDeviceToHost, s) != hipSuccess) return false;
    if (hipStreamSynchronize(s) != hipSuccess) return false;
    if (hipGetLastError() != hipSuccess) return false;
    if (count[kOpeningDepthMax + 1] != 0u) return false;
    for (int d = 0; d <= kOpeningDepthMax; d++)
        if (count[d] != kOpeningLevel[d]) return false;
    return true;
}

}  // namespace oth
