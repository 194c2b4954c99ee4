// split_tree_common.hpp — what the split search's tree (tree_core.hpp) and the
// split solver's (solve_tree_core.hpp) have in common, templated on the node
// type: the state word, the back-up, the window derivation, the placement of a
// node's children and the root's answer.  DESIGN.md §15 has the argument.
//
// A node type has the fields P, O, M (the mover's discs, the opponent's, the
// mover's moves), state, parent (slab index, -1 at the root), first_child,
// nchild, move, flags (bit kFinal) and snap; what else it carries (plies left
// and side, or empties) is its core's business, as are make_node, child_count,
// start_task, the statuses and the window's ends.
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

#ifdef __HIPCC__
#define OTHX_FN __device__ __forceinline__
#else
#define OTHX_FN inline
#endif

namespace othx {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr u32 kFinal = 1;  // neither side can move: the value is in the state word
constexpr u32 kNoMove = 255, kPassMove = 64;  // both rule sets' move codes

constexpr u64 kLimitBit = 1ull << 31;
constexpr u64 kCountMask = kLimitBit - 1;

OTHX_FN u64 pack(int best, u64 low) { return ((u64)(u32)best << 32) | low; }
OTHX_FN int best_of(u64 w) { return (int)(u32)(w >> 32); }
OTHX_FN u32 count_of(u64 w) { return (u32)(w & kCountMask); }

// write node i's `cnt` children at slab[first ..]: one for a pass, else one per
// move in ascending squares.  make(child, P, O, move, spent) fills a child in,
// `spent` the plies its edge costs (0 for a pass).  kInf: the window's end.
template <class R, int kInf, class Node, class Make>
OTHX_FN void place_children(Node* slab, const Node& x, u32 i, u32 first, u32 cnt, Make make) {
    if (x.M == 0) {
        make(slab[first], x.O, x.P, kPassMove, 0);
    } else {
        u32 k = first;
        for (u64 m = x.M; m; m &= m - 1, k++) {
            const u32 sq = R::lowest(m);
            const u64 f = R::flips(sq, x.P, x.O);
            make(slab[k], x.O & ~f, x.P | f | (1ull << sq), sq, 1);
        }
    }
    slab[i].first_child = first;
    slab[i].nchild = (uint8_t)cnt;
    slab[i].state = pack(-kInf, cnt);
}

template <class Node>
OTHX_FN bool is_task(const Node& x) {
    return !(x.flags & kFinal) && x.nchild == 0;
}

// fold the finished child's value v (from ITS mover's side) into node p's
// word; returns the new word
template <class A, class Node>
OTHX_FN u64 fold(Node* slab, u32 p, int v, u64 lim) {
    u64 old = A::load(&slab[p].state), nw;
    do {
        const int b = best_of(old);
        nw = pack(-v > b ? -v : b, ((old | lim) & kLimitBit) | (u64)(count_of(old) - 1u));
    } while (!A::cas(&slab[p].state, old, nw));
    return nw;
}

// task i (never the root) is finished with value v: carry it up as far as nodes
// complete.  True when the root completed.  Bounded by the tree's height.
template <class A, class Node>
OTHX_FN bool fold_up(Node* slab, u32 i, int v, u64 lim) {
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

// the window of task t from its ancestors' words, in t's mover's view, inside
// (-kInf, kInf): an ancestor an even number of edges up bounds alpha by its
// best, an odd one bounds beta by minus its best.  The ROOT hands down best - 1,
// so that a root child that ties the maximum still comes back exact (the tie
// rule).  With `shared` false the bests are the expansion's snapshot.
//
//
// kRootWindow (the split solver's; the split search leaves it off and compiles
// what it always did): (ra, rb) is the ROOT's own window, -kInf <= ra < rb <=
// kInf, and with the full one every task's window is what it is without the
// parameter.  The root is never cut off (all its children are resolved, so that
// the lowest square that reaches rb can be read off them): it hands down rb as
// one more bound, and max(ra, min(best, rb) - 1) for its best, so a root
// child's window is never empty and is (rb - 1, rb) once the root has reached rb.
template <class A, int kInf, bool kRootWindow = false, class Node>
OTHX_FN void window(Node* slab, u32 t, bool shared, int& alpha, int& beta, int ra = -kInf, int rb = kInf) {
    alpha = -kInf;
    beta = kInf;
    bool odd = true;
    for (int i = slab[t].parent; i >= 0; i = slab[i].parent, odd = !odd) {
        int b = shared ? best_of(A::load(&slab[i].state)) : (int)slab[i].snap;
        if constexpr (kRootWindow) {
            if (slab[i].parent < 0) {
                if (b > rb) b = rb;
                if (b > -kInf) b--;
                if (b < ra) b = ra;
                if (odd) {
                    if (-rb > alpha) alpha = -rb;
                } else if (rb < beta) {
                    beta = rb;
                }
            }
        } else {
            if (slab[i].parent < 0 && b > -kInf) b--;
        }
        if (odd) {
            if (-b < beta) beta = -b;
        } else if (b > alpha) {
            alpha = b;
        }
    }
}

// the completed root's answer; `done` and `limit` are the rule set's statuses
template <class A, class Node>
OTHX_FN void root_result(Node* slab, u32 done, u32 limit, int& value, u32& move, u32& status) {
    const u64 w = A::load(&slab[0].state);
    if (w & kLimitBit) {
        value = 0;
        move = kNoMove;
        status = limit;
        return;
    }
    value = best_of(w);
    status = done;
    if (slab[0].flags & kFinal) {
        move = kNoMove;
    } else if (slab[0].M == 0) {
        move = kPassMove;
    } else {
        move = kNoMove;
        const u32 f = slab[0].first_child, e = f + slab[0].nchild;
        for (u32 c = f; c < e; c++)
            if (-best_of(A::load(&slab[c].state)) == value) {
                move = slab[c].move;
                break;
            }
    }
}

}  // namespace othx
