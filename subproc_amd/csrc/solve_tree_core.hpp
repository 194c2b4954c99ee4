// solve_tree_core.hpp — the split solver's tree: tree_core.hpp's node layout,
// expansion, window derivation and back-up with the exact solver's semantics,
// written once for the device (solve_tree.hip) and the host
// (tools/diag/solve_tree_host.cpp).  DESIGN.md §17 has the argument (§15's,
// carried over).
//
// A position owns a slab of nodes.  Node 0 is the root; a round of expansion
// appends the children of every non-final node of the round before that still
// has more than `task_empties` empty squares, in parent order, ascending
// squares.  The root is expanded whatever its empties (a task is never the
// root, so that the root's move can be read off its children).  A node whose
// mover must pass gets ONE child, the same board with the other side to move,
// so EVERY edge of the tree negates.  A node where neither side can move is
// FINAL: its value, its mover's disc difference (no bonus for empties, no
// scale), is known when it is made.  The tasks are the nodes that are neither
// final nor expanded; each is searched by solve_core.hpp's advance() or
// solve_order_core.hpp's advance_ordered() and has at most 12 empties.
//
// One 64-bit state word per node is all that tasks share:
//   bits 63..32  best value so far, from the node's mover's side (int32, -65..64)
//   bit  31      a task below met the node limit (sticky on the way up)
//   bits 30..0   children not finished yet
// It is read and written by the atomics of the template parameter A only
// (agent scope on the device).  Everything else in a node is written by the
// expansion launch and only read afterwards.
#pragma once
#include <stdint.h>

#include "solve_core.hpp"

#ifdef __HIPCC__
#define OTHE_FN __device__ __forceinline__
#else
#define OTHE_FN inline
#endif

namespace othe {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr int kMaxEmpties = 16;         // OTHE_MAX_EMPTIES
constexpr u32 kNoRoom = 4;              // OTHE_NOROOM
constexpr int kMinNodes = 64;           // OTHE_MIN_NODES: the root's level always fits
// a placement and a pass alternate at worst, the root's round may be an extra one
constexpr int kMaxRounds = 2 * kMaxEmpties + 2;
// the window's ends: the solver's own root window (-65, 65), which the int8
// halves of a frame's packed window hold
constexpr int kInf = 65;

constexpr u32 kFinal = 1;  // neither side can move: the value is in the state word

constexpr u64 kLimitBit = 1ull << 31;
constexpr u64 kCountMask = kLimitBit - 1;

struct Node {
    u64 P, O, M;      // the mover's discs, the opponent's, the mover's moves
    u64 state;
    int32_t parent;   // slab index, -1 at the root
    u32 first_child;  // slab index of the first of nchild children (expanded nodes)
    uint8_t move;     // the square that made it, 64 for a pass, 255 at the root
    uint8_t emp;      // its empty squares
    uint8_t flags;
    uint8_t nchild;
    int32_t snap;     // best after the expansion's own back-up: the "nothing shared" windows
};
static_assert(sizeof(Node) == 48, "node layout");

OTHE_FN u64 pack(int best, u64 low) { return ((u64)(u32)best << 32) | low; }
OTHE_FN int best_of(u64 w) { return (int)(u32)(w >> 32); }
OTHE_FN u32 count_of(u64 w) { return (u32)(w & kCountMask); }

template <class R>
OTHE_FN void make_node(Node& c, u64 P, u64 O, int parent, u32 move) {
    const u64 m = R::moves(P, O);
    const bool over = m == 0 && R::moves(O, P) == 0;
    c.P = P;
    c.O = O;
    c.M = m;
    c.state = over ? pack(R::count(P) - R::count(O), 0) : pack(-kInf, 0);
    c.parent = parent;
    c.first_child = 0;
    c.move = (uint8_t)move;
    c.emp = (uint8_t)(64 - R::count(P | O));
    c.flags = (uint8_t)(over ? kFinal : 0u);
    c.nchild = 0;
    c.snap = -kInf;
}

// children a round makes below node x (0: it is final or small enough)
template <class R>
OTHE_FN u32 child_count(const Node& x, int task_empties) {
    if (x.flags & kFinal) return 0;
    if (x.parent >= 0 && (int)x.emp <= task_empties) return 0;
    return x.M ? (u32)R::count(x.M) : 1u;
}

// write node i's `cnt` children at slab[first ..]
template <class R>
OTHE_FN void expand(Node* slab, u32 i, u32 first, u32 cnt) {
    const Node x = slab[i];
    if (x.M == 0) {
        make_node<R>(slab[first], x.O, x.P, (int)i, oths::kPassMove);
    } else {
        u32 k = first;
        for (u64 m = x.M; m; m &= m - 1, k++) {
            const u32 sq = R::lowest(m);
            const u64 f = R::flips(sq, x.P, x.O);
            make_node<R>(slab[k], x.O & ~f, x.P | f | (1ull << sq), (int)i, sq);
        }
    }
    slab[i].first_child = first;
    slab[i].nchild = (uint8_t)cnt;
    slab[i].state = pack(-kInf, cnt);
}

OTHE_FN bool is_task(const Node& x) { return !(x.flags & kFinal) && x.nchild == 0; }

// fold the finished child's value v (from ITS mover's side) into node p's
// word; returns the new word
template <class A>
OTHE_FN u64 fold(Node* slab, u32 p, int v, u64 lim) {
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
OTHE_FN bool fold_up(Node* slab, u32 i, int v, u64 lim) {
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
// `shared` false the bests are the expansion's snapshot.  Both ends lie in
// -65..65.
template <class A>
OTHE_FN void window(Node* slab, u32 t, bool shared, int& alpha, int& beta) {
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

// a task enters the solver's state machine past its kRootNew step
OTHE_FN void start_task(oths::Lane& L, const Node& x, int alpha, int beta) {
    L.P = x.P;
    L.O = x.O;
    L.M = x.M;
    L.alpha = alpha;
    L.beta = beta;
    L.flags = x.M ? 0u : oths::kFresh;
    L.depth = 0;
    L.nodes = 0;
    L.root_mv = oths::kNoMove;
    L.best_mv = oths::kNoMove;
    L.value = 0;
    L.status = oths::kSolved;
}

// the completed root's answer
template <class A>
OTHE_FN void root_result(Node* slab, int& value, u32& move, u32& status) {
    const u64 w = A::load(&slab[0].state);
    if (w & kLimitBit) {
        value = 0;
        move = oths::kNoMove;
        status = oths::kLimit;
        return;
    }
    value = best_of(w);
    status = oths::kSolved;
    if (slab[0].flags & kFinal) {
        move = oths::kNoMove;
    } else if (slab[0].M == 0) {
        move = oths::kPassMove;
    } else {
        move = oths::kNoMove;
        const u32 f = slab[0].first_child, e = f + slab[0].nchild;
        for (u32 c = f; c < e; c++)
            if (-best_of(A::load(&slab[c].state)) == value) {
                move = slab[c].move;
                break;
            }
    }
}

}  // namespace othe
