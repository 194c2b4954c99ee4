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
// The state word that the tasks share, the back-up, the windows and the
// root's answer are split_tree_common.hpp's, which the split solver's tree
// (solve_tree_core.hpp) uses too; this file keeps what the search's tree alone
// has: a node with plies left and a side, its values' scale, its task.
#pragma once
#include <stdint.h>

#include "search_core.hpp"
#include "split_tree_common.hpp"

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

using othx::kFinal;           // flag 1
constexpr u32 kSideRoot = 2;  // the node's mover is the root mover

using othx::best_of;
using othx::count_of;
using othx::fold;
using othx::fold_up;
using othx::is_task;
using othx::kLimitBit;
using othx::pack;

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
static_assert(othx::kNoMove == othm::kNoMove && othx::kPassMove == othm::kPassMove, "move codes");

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
    othx::place_children<R, kInf>(slab, x, i, first, cnt, [&](Node& c, u64 P, u64 O, u32 move, int spent) {
        make_node<R>(c, P, O, (int)i, move, x.rem - spent, side);
    });
}

// split_tree_common.hpp's window, inside (-kInf, kInf)
template <class A>
OTHT_FN void window(Node* slab, u32 t, bool shared, int& alpha, int& beta) {
    othx::window<A, kInf>(slab, t, shared, alpha, beta);
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
    othx::root_result<A>(slab, othm::kSearched, othm::kLimit, value, move, status);
}

}  // namespace otht
