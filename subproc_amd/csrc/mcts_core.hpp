// mcts_core.hpp — the rule of the Monte Carlo tree search
// (include/othello_mcts.h) as code, written once for the device (mcts.hip) and
// the host (tools/diag/mcts_host.cpp): the selection score and its order, the
// child choice, the expansion test, the children, the back-up, the rows and
// the root's best move, and the ids of an iteration's playouts; and, for the
// trees that persist (include/othello_mcts_tree.h, mcts_tree.hip,
// tools/diag/mcts_tree_host.cpp), the re-rooting.
//
// search<R, A, K>() is the walk over one tree: init_root() and iterate().  R are the rules (moves, flips,
// lowest, count, kth), A is the tree's memory, K the wave:
//   A  pos / set_pos, visits_wins, n, d, link and their setters, add_stats, and
//      sync(): what lies between one phase's writes and the next phase's reads
//      of the same words by another lane;
//   K  how the 64 lanes of an iteration cooperate:
//        each(count, f)   f(k) for k = 0 .. count-1, lane k % 64 doing k;
//        pick(cnt, f)     f(k, fresh, score) for the children k < cnt; the
//                         first fresh one, else the best by better();
//        path_set / path_get, sync();
//        playout(...)     the iteration's 64 games and their sums.
// On the device K is the wave itself: every lane runs search() in lockstep,
// each() runs f for the lane's own k, pick() is a ballot and an argmax.  On
// the host search() runs once and K loops.  Everything outside f is uniform:
// the same value in every lane.  So the order of the phases, every index and
// every comparison are one text.
//
// The score is float32 from individually rounded operations: contraction is
// off in score(), and `/` and sqrt are IEEE on both sides (hipcc's defaults
// for HIP are the correctly rounded ones; the host build is compiled with
// -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define OTHU_FN __device__ __forceinline__
#else
#define OTHU_FN inline
#endif

namespace othu {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr u32 kMaxIterations = 65536;  // OTHU_MAX_ITERATIONS
constexpr u32 kMaxNodes = 1u << 20;    // OTHU_MAX_NODES
constexpr u32 kPathEntries = 132;      // OTHU_PATH_ENTRIES
constexpr u32 kSearched = 1, kInvalid = 2;  // OTHU_SEARCHED ..
constexpr u32 kNoMove = 255, kPassMove = 64;
constexpr u32 kLanes = 64;  // playouts per iteration, and the most children of a node

// a node's children: first | cnt << 20; 0: not expanded (node 0 is nobody's child)
constexpr int kCntShift = 20;
static_assert(kMaxNodes == 1u << kCntShift, "a node index fits below the count");
OTHU_FN u32 link_of(u32 first, u32 cnt) { return first | (cnt << kCntShift); }
OTHU_FN u32 link_first(u32 link) { return link & ((1u << kCntShift) - 1u); }
OTHU_FN u32 link_cnt(u32 link) { return link >> kCntShift; }

// the selection score of a visited child (n_c >= 1) below a parent whose
// visits' logarithm is log_nv
OTHU_FN float score(u32 s_c, u32 n_c, float log_nv, float c) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float mean = (float)s_c / (float)(128u * n_c);  // both exact: at most 2^23
    const float ratio = log_nv / (float)n_c;
    const float root = sqrtf(ratio);
    const float bonus = c * root;
    return mean + bonus;
}

// whether child a = (score, index) is chosen over b: a strict `>`, ties to the lowest index
OTHU_FN bool better(float sa, u32 ia, float sb, u32 ib) { return sa > sb || (sa == sb && ia < ib); }

// step 2's test: v has cnt children to make (0: terminal), n visits, and the tree has `nodes` of max_nodes
OTHU_FN bool may_expand(bool is_root, u32 n, u32 cnt, u32 nodes, u32 max_nodes) {
    return cnt != 0 && (is_root || n > 0) && nodes + cnt <= max_nodes;
}

// child k of (P to move, O) with move mask `legal` (0: the pass child), in ascending square order
template <class R>
OTHU_FN void make_child(u64 P, u64 O, u64 legal, u32 k, u64& cP, u64& cO) {
    cP = O;
    cO = P;
    if (legal) {
        const u32 sq = R::kth(legal, k);
        const u64 f = R::flips(sq, P, O);
        cP = O & ~f;
        cO = P | f | (1ull << sq);
    }
}

// step 4: what the node `up` levels above the leaf adds to its s and d
OTHU_FN u32 backed_w(u32 W, u32 up) { return (up & 1u) ? 128u - W : W; }
OTHU_FN int backed_d(int D, u32 up) { return (up & 1u) ? -D : D; }

// a game's half-points from its final disc difference
OTHU_FN u32 half_points(int dp) { return dp > 0 ? 2u : (dp == 0 ? 1u : 0u); }

// the global id of lane 0's playout in iteration t of position i (modulo 2^64)
OTHU_FN u64 playout_id0(u64 game_id0, u64 i, u32 iterations, u32 t) {
    return game_id0 + (i * (u64)iterations + (u64)t) * (u64)kLanes;
}

// the root's best move as a key whose maximum is the choice: most visits
// (<= 2^16), then more wins (<= 2^23), then the lowest square.  Bit 63 marks a
// legal square, so that one wins over "no move" (0) even unvisited.
OTHU_FN u64 move_key(u32 n, u32 s, u32 sq) {
    return (1ull << 63) | ((u64)n << 40) | ((u64)s << 8) | (u64)(63u - sq);
}
OTHU_FN u32 key_square(u64 key) { return 63u - (u32)(key & 63u); }

struct Params {
    u32 iterations, max_nodes;
    float explore;
    const float* log_table;  // [iterations + 1]
    u64 seed_state, game_id0;
};

// The root alone: node 0 = (P to move, O) with n = s = d = 0 and no children.
// Ends in a sync.
template <class A, class K>
OTHU_FN void init_root(A& tree, K& wave, u64 rootP, u64 rootO) {
    wave.each(1u, [&](u32) {
        tree.set_pos(0u, rootP, rootO);
        tree.set_stats(0u, 0u, 0u, 0);
        tree.set_link(0u, 0u);
    });
    tree.sync();
}

// `count` more iterations of steps 1 to 4 on a tree that holds `nodes` nodes.
// Iteration t = 0 .. count-1 plays the games of global ids
// id_base + (first + t) * 64 + lane (modulo 2^64); log_table has entries
// 0..table_last.  Every lane of K calls it with the same arguments.  Returns
// the tree's node count afterwards.  Ends in a sync.
template <class R, class A, class K>
OTHU_FN u32 iterate(A& tree, K& wave, u64 id_base, u64 first_iteration, u32 count, u32 nodes, u32 table_last,
                    const Params& p) {
    for (u32 t = 0; t < count; t++) {
        // 1. select
        u32 v = 0, depth = 0;
        wave.path_set(0u, 0u);
        for (;;) {
            const u32 link = tree.link(v);
            const u32 cnt = link_cnt(link), first = link_first(link);
            if (cnt == 0 || depth + 2u >= kPathEntries) break;  // (a path never gets that long: header)
            const u32 n_v = tree.n(v);
            const float log_nv = p.log_table[n_v <= table_last ? n_v : table_last];  // (n_v never passes it)
            const u32 k = wave.pick(cnt, [&](u32 c, bool& fresh, float& sc) {
                u32 n_c, s_c;
                tree.visits_wins(first + c, n_c, s_c);
                fresh = n_c == 0;
                sc = fresh ? 0.0f : score(s_c, n_c, log_nv, p.explore);
            });
            v = first + k;
            depth++;
            wave.path_set(depth, v);
        }
        // 2. expand
        u64 P, O;
        tree.pos(v, P, O);
        const u64 legal = R::moves(P, O);
        const u32 cnt = legal ? (u32)R::count(legal) : (R::moves(O, P) ? 1u : 0u);
        if (tree.link(v) == 0u && may_expand(v == 0u, tree.n(v), cnt, nodes, p.max_nodes)) {
            const u32 first = nodes;
            wave.each(cnt, [&](u32 c) {
                u64 cP, cO;
                make_child<R>(P, O, legal, c, cP, cO);
                tree.set_pos(first + c, cP, cO);
                tree.set_stats(first + c, 0u, 0u, 0);
                tree.set_link(first + c, 0u);
            });
            wave.each(1u, [&](u32) { tree.set_link(v, link_of(first, cnt)); });
            make_child<R>(P, O, legal, 0u, P, O);  // on to the first child
            v = first;
            nodes += cnt;
            depth++;
            wave.path_set(depth, v);
        }
        // 3. play out
        u32 W;
        int D;
        wave.playout(P, O, id_base + (first_iteration + (u64)t) * (u64)kLanes, p.seed_state, W, D);
        // 4. back up: a path's nodes are distinct, so each is one lane's
        tree.sync();
        wave.sync();
        wave.each(depth + 1u, [&](u32 k) {
            const u32 up = depth - k;
            tree.add_stats(wave.path_get(k), 1u, backed_w(W, up), backed_d(D, up));
        });
        tree.sync();
        wave.sync();
    }
    return nodes;
}

// One tree: `iterations` iterations from the root (P to move, O), the position
// of index i.  Every lane of K calls it with the same arguments.  Returns the
// number of nodes made.
template <class R, class A, class K>
OTHU_FN u32 search(A& tree, K& wave, u64 rootP, u64 rootO, u64 i, const Params& p) {
    init_root(tree, wave, rootP, rootO);
    return iterate<R>(tree, wave, playout_id0(p.game_id0, i, p.iterations, 0u), 0u, p.iterations, 1u, p.iterations, p);
}

// ---- trees that persist (include/othello_mcts_tree.h) ----

// node `to_v` of `to` becomes node `from_v` of `from`, its children word included
template <class A, class B>
OTHU_FN void copy_node(B& to, u32 to_v, const A& from, u32 from_v) {
    u64 P, O;
    u32 n, s;
    from.pos(from_v, P, O);
    from.visits_wins(from_v, n, s);
    to.set_pos(to_v, P, O);
    to.set_stats(to_v, n, s, from.d(from_v));
    to.set_link(to_v, from.link(from_v));
}

// Re-root: the subtree of `tree` below node c becomes the whole tree, c as
// node 0, every node with its n, s, d.  The subtree is copied breadth first
// into `half` (room for as many nodes as the tree holds), which is its own
// queue: the nodes [head, tail) of `half` are copied but still carry their
// children word in the OLD numbering.  A turn of the loop takes up to 64 of
// them, gives their children blocks consecutive places from `tail` on, in queue
// order (K's scan), copies the blocks and rewrites the words; then `half` is
// copied back.  Every node is read and written twice: linear in the node
// count.  A block stays contiguous and in its order, and a parent precedes its
// children, which is all the walk asks of a numbering.  Returns the new node
// count.  Ends in a sync.
//   K::scan(count, f)   f(k, word, weight) for k < count <= 64; keeps word_k
//                       and the sum of the weights below k, returns the total;
//   K::scan_word(k), K::scan_below(k)   those, for a uniform k.
template <class A, class B, class K>
OTHU_FN u32 compact(A& tree, B& half, K& wave, u32 c, u32 room) {
    wave.each(1u, [&](u32) { copy_node(half, 0u, tree, c); });
    half.sync();
    u32 head = 0, tail = 1;
    while (head < tail) {
        const u32 take = tail - head < kLanes ? tail - head : kLanes;
        const u32 total = wave.scan(take, [&](u32 k, u32& word, u32& weight) {
            word = half.link(head + k);
            weight = link_cnt(word);
        });
        if (tail + total > room) break;  // (never in a tree this code made: `half` is not written past its end)
        for (u32 k = 0; k < take; k++) {
            const u32 word = wave.scan_word(k);
            const u32 cnt = link_cnt(word), first = link_first(word), dst = tail + wave.scan_below(k);
            if (cnt == 0) continue;
            wave.each(cnt, [&](u32 j) { copy_node(half, dst + j, tree, first + j); });
            wave.each(1u, [&](u32) { half.set_link(head + k, link_of(dst, cnt)); });
        }
        head += take;
        tail += total;
        half.sync();
    }
    wave.each(tail, [&](u32 k) { copy_node(tree, k, half, k); });
    tree.sync();
    return tail;
}

// whether `move` may be played at the root (P to move, O): a legal square, or
// the pass where the mover has no move and the other side has one
template <class R>
OTHU_FN bool may_play(u64 P, u64 O, u32 move) {
    const u64 legal = R::moves(P, O);
    if (move < 64u) return (legal >> move) & 1ull;
    return move == kPassMove && legal == 0 && R::moves(O, P) != 0;
}

// Advance the tree's root by `move` (may_play() holds).  keep and an expanded
// root: compact() below the child the move reaches.  Otherwise the child
// position alone.  Returns the new node count.  Ends in a sync.
template <class R, class A, class B, class K>
OTHU_FN u32 advance(A& tree, B& half, K& wave, u32 move, bool keep, u32 room) {
    u64 P, O;
    tree.pos(0u, P, O);
    const u64 legal = R::moves(P, O);
    const u32 link = tree.link(0u);
    const u32 k = legal ? (u32)R::count(legal & ((1ull << (move & 63u)) - 1ull)) : 0u;
    if (keep && link_cnt(link)) return compact(tree, half, wave, link_first(link) + k, room);
    u64 cP, cO;
    make_child<R>(P, O, legal, k, cP, cO);
    tree.sync();  // (every lane has read the root)
    init_root(tree, wave, cP, cO);
    return 1u;
}

// The entries of a finished tree's rows at square sq: n, s, d of the root
// child reached by sq, 0 elsewhere.  Returns the square's key for best_move
// (0: not a move).
template <class R, class A>
OTHU_FN u64 root_entry(A& tree, u64 legal, u32 sq, u32& n, u32& s, int& d) {
    n = 0, s = 0, d = 0;
    if (!((legal >> sq) & 1ull)) return 0;
    const u32 link = tree.link(0u);
    if (link_cnt(link)) {
        const u32 c = link_first(link) + (u32)R::count(legal & ((1ull << sq) - 1ull));
        tree.visits_wins(c, n, s);
        d = tree.d(c);
    }
    return move_key(n, s, sq);
}

// best_move from the largest key of the 64 squares (0: no legal square)
template <class R>
OTHU_FN u32 best_move_of(u64 best_key, u64 rootP, u64 rootO) {
    if (best_key) return key_square(best_key);
    return R::moves(rootO, rootP) ? kPassMove : kNoMove;
}

}  // namespace othu
