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
// The state word that the tasks share (its best value here in -65..64), the
// back-up, the windows and the root's answer are split_tree_common.hpp's; this
// file keeps what the solver's tree alone has: a node with its empties, values
// without a scale, the window's ends, its task.
#pragma once
#include <stdint.h>

#include "solve_core.hpp"
#include "split_tree_common.hpp"

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

using othx::best_of;
using othx::count_of;
using othx::fold;
using othx::fold_up;
using othx::is_task;
using othx::kFinal;
using othx::kLimitBit;
using othx::pack;

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
static_assert(othx::kNoMove == oths::kNoMove && othx::kPassMove == oths::kPassMove, "move codes");

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
    othx::place_children<R, kInf>(slab, x, i, first, cnt,
                                  [&](Node& c, u64 P, u64 O, u32 move, int) { make_node<R>(c, P, O, (int)i, move); });
}

// split_tree_common.hpp's window; both ends lie in -65..65
template <class A>
OTHE_FN void window(Node* slab, u32 t, bool shared, int& alpha, int& beta) {
    othx::window<A, kInf>(slab, t, shared, alpha, beta);
}

// the same under the root's own window (ra, rb); with the full
// one it computes what window() does
template <class A>
OTHE_FN void window_rooted(Node* slab, u32 t, bool shared, int& alpha, int& beta, int ra, int rb) {
    othx::window<A, kInf, true>(slab, t, shared, alpha, beta, ra, rb);
}

// the root's window in one word (a position's header keeps it): the int8 halves
// of a frame's packed window
OTHE_FN u32 pack_window(int ra, int rb) { return (u32)(ra & 0xFF) | ((u32)(rb & 0xFF) << 8); }
OTHE_FN int window_alpha(u32 w) { return (int)(int8_t)(w & 0xFF); }
OTHE_FN int window_beta(u32 w) { return (int)(int8_t)((w >> 8) & 0xFF); }

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
    othx::root_result<A>(slab, oths::kSolved, oths::kLimit, value, move, status);
}

// the completed root's answer under its window (ra, rb): the value clamped, and
// for a root that has moves the lowest square whose child reaches the value
// (the lowest maximiser inside the window, the lowest move that reaches rb on a
// fail-high), none when no move beats ra.  With the full window it is
// root_result()'s answer.
template <class A>
OTHE_FN void root_result_window(Node* slab, int& value, u32& move, u32& status, int ra, int rb) {
    othx::root_result<A>(slab, oths::kSolved, oths::kLimit, value, move, status);
    if (status != oths::kSolved) return;
    const int best = value;
    value = oths::clamp_to_window(best, ra, rb);
    if ((slab[0].flags & kFinal) || slab[0].M == 0) return;
    move = oths::kNoMove;
    if (best <= ra) return;
    const u32 f = slab[0].first_child, e = f + slab[0].nchild;
    for (u32 c = f; c < e; c++)
        if (-best_of(A::load(&slab[c].state)) >= value) {
            move = slab[c].move;
            break;
        }
}

}  // namespace othe
