// mcts_wide_host.cpp — the wide Monte Carlo tree search
// (include/othello_mcts_wide.h) on the host: the very rounds the
// device runs (mcts_wide_core.hpp's search_wide() over mcts_core.hpp's score,
// child choice, expansion test and back-up) with mcts_host.cpp's plain C++
// rules, arrays, loops and random playout.  The block's waves are loops: the
// walkers run one after another, then every walker's games and back-up.
//
// Its use is mcts_host.cpp's first: the rule's code runs under
// -fsanitize=address,undefined against tests/mcts_wide_ref.py before any GPU run.
//
// build:  g++ -O2 -std=c++17 -ffp-contract=off -fopenmp -o tools/diag/mcts_wide_host tools/diag/mcts_wide_host.cpp
//         (-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all)
// run:    mcts_wide_host IN OUT rounds leaves explore_bits seed game_id0 max_nodes [threads=16]
//   IN, explore_bits, OUT: mcts_host.cpp's, the table with rounds * leaves + 1 lines
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../subproc_amd/csrc/mcts_wide_core.hpp"
#include "host_io.hpp"
#include "mcts_host_common.hpp"

// the block of mcts_wide_core.hpp: one HostWave that is every wave in turn
struct HostBlock : HostWave {
    u32 paths[othu::kMaxLeaves][othu::kPathEntries];
    u64 leafP[othu::kMaxLeaves], leafO[othu::kMaxLeaves];
    u32 depths[othu::kMaxLeaves];
    template <class F>
    void walkers(u32 count, F f) {
        for (u32 w = 0; w < count; w++) f(w);
    }
    template <class F>
    void waves(u32 count, F f) {
        for (u32 w = 0; w < count; w++) f(w);
    }
    void barrier() const {}
    void path_set(u32 w, u32 k, u32 v) {
        if (k < othu::kPathEntries) paths[w][k] = v;
    }
    u32 path_get(u32 w, u32 k) const { return paths[w][k < othu::kPathEntries ? k : 0]; }
    void leaf_set(u32 w, u64 P, u64 O, u32 depth) { leafP[w] = P, leafO[w] = O, depths[w] = depth; }
    void leaf_get(u32 w, u64& P, u64& O, u32& depth) const { P = leafP[w], O = leafO[w], depth = depths[w]; }
};

struct Row {
    u32 status = othu::kInvalid, best = othu::kNoMove, nodes = 0, root_wins = 0;
    int root_diffs = 0;
    u32 visits[64] = {}, wins[64] = {};
    int diffs[64] = {};
};

int main(int argc, char** argv) {
    if (argc < 9) usage(argv[0], "IN OUT rounds leaves explore_bits seed game_id0 max_nodes [threads=16]");
    const long R = atol(argv[3]), L = atol(argv[4]);
    const u32 cbits = (u32)strtoul(argv[5], nullptr, 16);
    const u64 seed = strtoull(argv[6], nullptr, 0), game_id0 = strtoull(argv[7], nullptr, 0);
    const long M = atol(argv[8]);
    const int threads = argc > 9 ? atoi(argv[9]) : 16;
    if (L < 1 || L > (long)othu::kMaxLeaves || R < 1 || R > (long)othu::kMaxIterations ||
        R * L > (long)othu::kMaxIterations || M < 1 || M > (long)othu::kMaxNodes || threads < 1)
        return 2;
    float c;
    memcpy(&c, &cbits, 4);
    std::vector<Pos> pos;
    std::vector<float> table;
    read_trees(argv[1], 0, pos, table);
    if ((long)table.size() != R * L + 1) return 2;
    const long n = (long)pos.size();
    std::vector<Row> rows(n);
    othu::Params p;
    p.iterations = (u32)R;
    p.max_nodes = (u32)M;
    p.explore = c;
    p.log_table = table.data();
    p.seed_state = othp::seed_state(seed);
    p.game_id0 = game_id0;
    u64 plies = 0, wave_plies = 0;
    (void)threads;
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads) reduction(+ : plies, wave_plies)
    for (long i = 0; i < n; i++) {
        const Pos& q = pos[i];
        Row& r = rows[i];
        if (q.black & q.white) continue;
        const u64 P = q.mover(), O = q.other();
        HostTree tree((u32)M);
        HostBlock block;
        r.nodes = othu::search_wide<Rules>(tree, block, P, O, (u64)i, (u32)L, p);
        plies += block.plies;
        wave_plies += block.wave_plies;
        const u64 legal = Rules::moves(P, O);
        u64 best = 0;
        for (u32 sq = 0; sq < 64; sq++) {
            const u64 key = othu::root_entry<Rules>(tree, legal, sq, r.visits[sq], r.wins[sq], r.diffs[sq]);
            if (key > best) best = key;
        }
        r.best = othu::best_move_of<Rules>(best, P, O);
        r.root_wins = 128u * tree.n(0) - tree.ss[0];
        r.root_diffs = -tree.d(0);
        r.status = othu::kSearched;
    }
    FILE* o = open_or_exit(argv[2], "w");
    for (long i = 0; i < n; i++) {
        const Row& r = rows[i];
        fprintf(o, "%u %u %u %u %d", r.status, r.best, r.nodes, r.root_wins, r.root_diffs);
        for (int s = 0; s < 64; s++) fprintf(o, " %u", r.visits[s]);
        for (int s = 0; s < 64; s++) fprintf(o, " %u", r.wins[s]);
        for (int s = 0; s < 64; s++) fprintf(o, " %d", r.diffs[s]);
        fprintf(o, "\n");
    }
    fprintf(o, "plies %llu wave_plies %llu\n", (unsigned long long)plies, (unsigned long long)wave_plies);
    fclose(o);
    return 0;
}
