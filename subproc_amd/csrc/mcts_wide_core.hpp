// mcts_wide_core.hpp — the round of the wide Monte Carlo tree search
// (include/othello_mcts_wide.h) as code, written once for the device
// (mcts_wide.hip) and the host (tools/diag/mcts_wide_host.cpp).  The score, the
// child choice, the expansion test, the children, the back-up's signs, the rows
// and the best move are mcts_core.hpp's; only the iteration is new.
//
// search_wide<R, A, K>() is the walk over one tree.  R and A are mcts_core.hpp's
// rules and tree memory; A gains
//   mark(v)             n += 1, by the one wave that selects;
//   add_result(v, s, d) s += s, d += d, by any wave at any time of the back-up
//                       phase (integer adds: the order does not matter);
// K is the block of L waves:
//   walkers(L, f)       f(w) for w = 0 .. L-1 in this order, by the selecting
//                       wave alone;
//   waves(L, f)         f(w) once for every w < L, wave w doing w;
//   barrier()           what lies between one phase's writes and the next
//                       phase's reads of the same words by another wave;
//   each, pick, sync, playout   as mcts_core.hpp's K, for the calling wave;
//   path_set / path_get (w, k), leaf_set / leaf_get (w): walker w's path and
//                       leaf, written in phase A, read in phases B and C.
// On the device every lane of the block runs search_wide() and K masks; on the
// host it runs once and K loops.  Everything outside f is uniform in a wave.
#pragma once
#include "mcts_core.hpp"

namespace othu {

constexpr u32 kMaxLeaves = 16;  // OTHV_MAX_LEAVES

// the global id of lane 0's playout for walker w of round r of position i (modulo 2^64)
OTHU_FN u64 wide_playout_id0(u64 game_id0, u64 i, u32 rounds, u32 leaves, u32 r, u32 w) {
    return game_id0 + ((i * (u64)rounds + (u64)r) * (u64)leaves + (u64)w) * (u64)kLanes;
}

// One tree: p.iterations rounds of `leaves` walkers from the root (P to move,
// O), the position of index i; log_table has entries 0 .. iterations * leaves.
// Every lane of K calls it with the same arguments.  Returns the number of
// nodes made: in the selecting wave only.  Ends in a barrier.
template <class R, class A, class K>
OTHU_FN u32 search_wide(A& tree, K& block, u64 rootP, u64 rootO, u64 i, u32 leaves, const Params& p) {
    const u32 table_last = p.iterations * leaves;
    u32 nodes = 1;
    block.walkers(1u, [&](u32) { init_root(tree, block, rootP, rootO); });
    for (u32 r = 0; r < p.iterations; r++) {
        // A. the walkers, one after another
        block.walkers(leaves, [&](u32 w) {
            // 1. select
            u32 v = 0, depth = 0;
            block.path_set(w, 0u, 0u);
            for (;;) {
                const u32 link = tree.link(v);
                const u32 cnt = link_cnt(link), first = link_first(link);
                if (cnt == 0 || depth + 2u >= kPathEntries) break;  // (a path never gets that long)
                const u32 n_v = tree.n(v);
                const float log_nv = p.log_table[n_v <= table_last ? n_v : table_last];  // (n_v never passes it)
                const u32 k = block.pick(cnt, [&](u32 c, bool& fresh, float& sc) {
                    u32 n_c, s_c;
                    tree.visits_wins(first + c, n_c, s_c);
                    fresh = n_c == 0;
                    sc = fresh ? 0.0f : score(s_c, n_c, log_nv, p.explore);
                });
                v = first + k;
                depth++;
                block.path_set(w, depth, v);
            }
            // 2. expand
            u64 P, O;
            tree.pos(v, P, O);
            const u64 legal = R::moves(P, O);
            const u32 cnt = legal ? (u32)R::count(legal) : (R::moves(O, P) ? 1u : 0u);
            if (tree.link(v) == 0u && may_expand(v == 0u, tree.n(v), cnt, nodes, p.max_nodes)) {
                const u32 first = nodes;
                block.each(cnt, [&](u32 c) {
                    u64 cP, cO;
                    make_child<R>(P, O, legal, c, cP, cO);
                    tree.set_pos(first + c, cP, cO);
                    tree.set_stats(first + c, 0u, 0u, 0);
                    tree.set_link(first + c, 0u);
                });
                block.each(1u, [&](u32) { tree.set_link(v, link_of(first, cnt)); });
                make_child<R>(P, O, legal, 0u, P, O);  // on to the first child
                v = first;
                nodes += cnt;
                depth++;
                block.path_set(w, depth, v);
            }
            block.leaf_set(w, P, O, depth);
            // 3. mark: a path's nodes are distinct, so each is one lane's
            tree.sync();
            block.sync();
            block.each(depth + 1u, [&](u32 k) { tree.mark(block.path_get(w, k)); });
            tree.sync();
        });
        block.barrier();
        // B, C. play out and back up: wave w has walker w
        block.waves(leaves, [&](u32 w) {
            u64 P, O;
            u32 depth;
            block.leaf_get(w, P, O, depth);
            u32 W;
            int D;
            block.playout(P, O, wide_playout_id0(p.game_id0, i, p.iterations, leaves, r, w), p.seed_state, W, D);
            block.each(depth + 1u, [&](u32 k) {
                const u32 up = depth - k;
                tree.add_result(block.path_get(w, k), backed_w(W, up), backed_d(D, up));
            });
        });
        block.barrier();
    }
    return nodes;
}

}  // namespace othu
