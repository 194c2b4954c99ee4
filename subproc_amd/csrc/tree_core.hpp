// tree_core.hpp — the split search's tree: node layout, expansion of one node,
// window derivation and back-up, written once for the device (tree.hip) and
// the host (tools/diag/tree_host.cpp).  DESIGN.md §15 has the argument.
//
// A position owns a slab of nodes.  Node 0 is the root; a round of expansion
// appends the children of every node of the round before that still has more
// than `target = depth - split` plies left, in parent order, ascending squares.
// A node whose mover must pass gets ONE child, the same board with the other
// side to move and the same `rem`, so EVERY edge of the tree negates (the
// state machine's kPassed is the same thing seen from inside one frame).  A
// node where neither side can move is FINAL: its value is known when it is
// made.  The tasks are the nodes that are neither final nor expanded; each is
// searched by search_core.hpp's advance() with `rem` plies (1..8).
//
// One 64-bit state word per node is all that tasks share:
//   bits 63..32  best value so far, from the node's mover's side (int32)
//   bit  31      a task below met the node limit (sticky on the way up)
//   bits 30..0   children not finished yet
// It is read and written by the atomics of the template parameter A only
// (agent scope on the device).  Everything else in a node is written by the
// expansion launch and only read afterwards.
#pragma once
#include <stdint.h>

#include "search_core.hpp"

#ifdef __HIPCC__
#define OTHT_FN __device__ __forceinline__
#else
#define OTHT_FN inline
#endif

namespace otht {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr int kMaxSplit = 4;            // OTHT_MAX_SPLIT
constexpr u32 kNoRoom = 4;              // OTHT_NOROOM
constexpr int kMinNodes = 64;           // nodes_per_position's lower bound: the root's level always fits
constexpr int kMaxRounds = 2 * kMaxSplit + 1;  // a pass and a placement alternate at worst
constexpr int kInf = othm::kInf;

constexpr u32 kFinal = 1;     // neither side can move: the value is in the state word
constexpr u32 kSideRoot = 2;  // the node's mover is the root mover

constexpr u64 kLimitBit = 1ull << 31;
constexpr u64 kCountMask = kLimitBit - 1;

struct Node {
    u64 P, O, M;      // the mover's discs, the opponent's, the mover's moves
    u64 state;
    int32_t parent;   // slab index, -1 at the root
    u32 first_child;  // slab index of the first of nchild children (expanded nodes)
    uint8_t move;     // the square that made it, 64 for a pass, 255 at the root
    uint8_t rem;      // plies left below it
    uint8_t flags;
    uint8_t nchild;
    int32_t snap;     // best after the expansion's own back-up: the "nothing shared" windows
};
static_assert(sizeof(Node) == 48, "node layout");

OTHT_FN u64 pack(int best, u64 low) { return ((u64)(u32)best << 32) | low; }
OTHT_FN int best_of(u64 w) { return (int)(u32)(w >> 32); }
OTHT_FN u32 count_of(u64 w) { return (u32)(w & kCountMask); }

template <class R>
OTHT_FN void make_node(Node& c, u64 P, u64 O, int parent, u32 move, int rem, u32 side) {
    const u64 m = R::moves(P, O);
    const bool over = m == 0 && R::moves(O, P) == 0;
    c.P = P;
    c.O = O;
    c.M = m;
    c.state = over ? pack(othm::kTerminal * (R::count(P) - R::count(O)), 0) : pack(-kInf, 0);
    c.parent = parent;
    c.first_child = 0;
    c.move = (uint8_t)move;
    c.rem = (uint8_t)rem;
    c.flags = (uint8_t)((over ? kFinal : 0u) | side);
    c.nchild = 0;
    c.snap = -kInf;
}

// children a round makes below node x (0: it is final or deep enough)
template <class R>
OTHT_FN u32 child_count(const Node& x, int target) {
    if ((x.flags & kFinal) || (int)x.rem <= target) return 0;
    return x.M ? (u32)R::count(x.M) : 1u;
}

// write node i's `cnt` children at slab[first ..]
template <class R>
OTHT_FN void expand(Node* slab, u32 i, u32 first, u32 cnt) {
    const Node x = slab[i];
    const u32 side = (x.flags & kSideRoot) ^ kSideRoot;
    if (x.M == 0) {
        make_node<R>(slab[first], x.O, x.P, (int)i, othm::kPassMove, x.rem, side);
    } else {
        u32 k = first;
        for (u64 m = x.M; m; m &= m - 1, k++) {
            const u32 sq = R::lowest(m);
            const u64 f = R::flips(sq, x.P, x.O);
            make_node<R>(slab[k], x.O & ~f, x.P | f | (1ull << sq), (int)i, sq, x.rem - 1, side);
        }
    }
    slab[i].first_child = first;
    slab[i].nchild = (uint8_t)cnt;
    slab[i].state = pack(-kInf, cnt);
}

OTHT_FN bool is_task(const Node& x) { return !(x.flags & kFinal) && x.nchild == 0; }

// fold the finished child's value v (from ITS mover's side) into node p's
// word; returns the new word
template <class A>
OTHT_FN u64 fold(Node* slab, u32 p, int v, u64 lim) {
    u64 old = A::load(&slab[p].state), nw;
    do {
        const int b = best_of(old);
        nw = pack(-v > b ? -v : b, ((old | lim) & kLimitBit) | (u64)(count_of(old) - 1u));
    } while (!A::cas(&slab[p].state, old, nw));
    return nw;
}

// task i (never the root) is finished with value v: carry it up as far as nodes
// complete.  True when the root completed.  Bounded by the tree's height.
template <class A>
OTHT_FN bool fold_up(Node* slab, u32 i, int v, u64 lim) {
    A::store(&slab[i].state, pack(v, lim));  // a task's own word: the root's scan reads its children's
    for (;;) {
        const u32 p = (u32)slab[i].parent;
        const u64 w = fold<A>(slab, p, v, lim);
        if (count_of(w) != 0) return false;
        if (slab[p].parent < 0) return true;
        i = p;
        v = best_of(w);
        lim = w & kLimitBit;
    }
}

// the window of task t from its ancestors' words, in t's mover's view: an
// ancestor an even number of edges up bounds alpha by its best, an odd one
// bounds beta by minus its best.  The ROOT hands down best - 1, so that a root
// child that ties the maximum still comes back exact (the tie rule).  With
// `shared` false the bests are the expansion's snapshot.
template <class A>
OTHT_FN void window(Node* slab, u32 t, bool shared, int& alpha, int& beta) {
    alpha = -kInf;
    beta = kInf;
    bool odd = true;
    for (int i = slab[t].parent; i >= 0; i = slab[i].parent, odd = !odd) {
        int b = shared ? best_of(A::load(&slab[i].state)) : (int)slab[i].snap;
        if (slab[i].parent < 0 && b > -kInf) b--;
        if (odd) {
            if (-b < beta) beta = -b;
        } else if (b > alpha) {
            alpha = b;
        }
    }
}

// a task enters the state machine past its kRootNew step
OTHT_FN void start_task(othm::Lane& L, const Node& x, int alpha, int beta) {
    L.P = x.P;
    L.O = x.O;
    L.M = x.M;
    L.alpha = alpha;
    L.beta = beta;
    L.flags = ((x.flags & kSideRoot) ? othm::kRootSide : 0u) | (x.M ? 0u : othm::kFresh);
    L.rem = x.rem;
    L.depth = 0;
    L.nodes = 0;
    L.root_mv = othm::kNoMove;
    L.best_mv = othm::kNoMove;
    L.value = 0;
    L.status = othm::kSearched;
}

// the completed root's answer
template <class A>
OTHT_FN void root_result(Node* slab, int& value, u32& move, u32& status) {
    const u64 w = A::load(&slab[0].state);
    if (w & kLimitBit) {
        value = 0;
        move = othm::kNoMove;
        status = othm::kLimit;
        return;
    }
    value = best_of(w);
    status = othm::kSearched;
    if (slab[0].flags & kFinal) {
        move = othm::kNoMove;
    } else if (slab[0].M == 0) {
        move = othm::kPassMove;
    } else {
        move = othm::kNoMove;
        const u32 f = slab[0].first_child, e = f + slab[0].nchild;
        for (u32 c = f; c < e; c++)
            if (-best_of(A::load(&slab[c].state)) == value) {
                move = slab[c].move;
                break;
            }
    }
}

}  // namespace otht
