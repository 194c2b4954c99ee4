// mcts_host.cpp — the Monte Carlo tree search (include/othello_mcts.h,
// DESIGN.md §28) on the host: the very walk the device runs
// (mcts_core.hpp's search(): score, child choice, expansion test, back-up) with
// a plain C++ statement of the rules, arrays for the tree, loops for the wave's
// collectives and a plain C++ random playout over DESIGN.md §4's draws.
//
// Two uses, as perft_host.cpp's:
//   * the rule's code can be run under -fsanitize=address,undefined and compared
//     against tests/mcts_ref.py before any GPU run;
//   * with threads it is the host baseline of tools/mcts_bench.py.
//
// build:  g++ -O2 -std=c++17 -ffp-contract=off -fopenmp -o tools/diag/mcts_host tools/diag/mcts_host.cpp
//         (-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all)
// run:    mcts_host IN OUT iterations explore_bits seed game_id0 max_nodes [threads=16]
//   IN : one position per line, "<black hex> <white hex> <turn>", and the
//        table as iterations + 1 lines "L <float32 bits hex>" in order
//   explore_bits: the exploration constant's float32 bits, hex
//   OUT: one line per position, "<status> <best_move> <nodes> <root_wins>
//        <root_diffs>", then the 64 visits, the 64 wins and the 64 diffs; then
//        one line "plies <env-steps of all playouts> wave_plies <the sum over
//        the iterations of their longest game>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_io.hpp"
#include "mcts_host_common.hpp"

struct Row {
    u32 status = othu::kInvalid, best = othu::kNoMove, nodes = 0, root_wins = 0;
    int root_diffs = 0;
    u32 visits[64] = {}, wins[64] = {};
    int diffs[64] = {};
};

int main(int argc, char** argv) {
    if (argc < 8) usage(argv[0], "IN OUT iterations explore_bits seed game_id0 max_nodes [threads=16]");
    const long T = atol(argv[3]);
    const u32 cbits = (u32)strtoul(argv[4], nullptr, 16);
    const u64 seed = strtoull(argv[5], nullptr, 0), game_id0 = strtoull(argv[6], nullptr, 0);
    const long M = atol(argv[7]);
    const int threads = argc > 8 ? atoi(argv[8]) : 16;
    if (T < 1 || T > (long)othu::kMaxIterations || M < 1 || M > (long)othu::kMaxNodes || threads < 1) return 2;
    float c;
    memcpy(&c, &cbits, 4);
    std::vector<Pos> pos;
    std::vector<float> table;
    read_trees(argv[1], 0, pos, table);
    if ((long)table.size() != T + 1) return 2;
    const long n = (long)pos.size();
    std::vector<Row> rows(n);
    othu::Params p;
    p.iterations = (u32)T;
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
        HostWave wave;
        r.nodes = othu::search<Rules>(tree, wave, P, O, (u64)i, p);
        plies += wave.plies;
        wave_plies += wave.wave_plies;
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
