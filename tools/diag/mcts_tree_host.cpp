// mcts_tree_host.cpp — the Monte Carlo search trees that persist
// (include/othello_mcts_tree.h) on the host: the text the device
// runs (mcts_core.hpp's init_root(), iterate(), advance() and compact()) over
// mcts_host_common.hpp's arrays and loops, driven by a script of operations.
//
// The re-rooting is index arithmetic over a slab, so this is the build to run
// under -fsanitize=address,undefined and to compare against
// tests/mcts_tree_ref.py before any GPU run.
//
// build:  g++ -O2 -std=c++17 -ffp-contract=off -o tools/diag/mcts_tree_host tools/diag/mcts_tree_host.cpp
//         (-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all)
// run:    mcts_tree_host IN SCRIPT OUT explore_bits seed max_nodes
//   IN    : one tree per line, "<black hex> <white hex> <turn> <id_base>", and
//           the table as lines "L <float32 bits hex>" for n = 0, 1, ...: the
//           library's table has OTHU_MAX_ITERATIONS + 1 entries, this one as
//           many as the run needs (an n_v past its end takes the last entry)
//   SCRIPT: one operation per line, applied to every tree
//             init
//             search T | search T0 T1 ...     (one count, or one per tree)
//             advance KEEP M0 M1 ...          (one move code per tree)
//             advance KEEP best | last        (the tree's best move | the root
//                                             mover's last legal square, 64
//                                             where it must pass, 255 where the
//                                             game is over)
//             rows
//             dump
//   OUT   : what the operations answer, in order, one line per tree:
//             search, rows: "R <status> <best_move> <nodes> <root_wins>
//                    <root_diffs> <ran> <black hex> <white hex> <turn>", the 64
//                    visits, the 64 wins, the 64 diffs
//             advance: "A <status> <move>"
//             dump: "T <nodes> <played>", then per node in breadth-first order
//                    from the root "<P hex> <O hex> <n> <s> <d> <children>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/othello_mcts_tree.h"
#include "host_io.hpp"
#include "mcts_host_common.hpp"

struct Tree {
    HostTree nodes, half;
    u64 id_base = 0, played = 0;
    u32 count = 0, turn = 1, status = OTHR_INVALID, ran = 0;
    explicit Tree(u32 M) : nodes(M), half(M) {}
};

static u32 best_move(Tree& t, u32* visits, u32* wins, int* diffs) {
    u64 P, O;
    t.nodes.pos(0, P, O);
    const u64 legal = Rules::moves(P, O);
    u64 best = 0;
    for (u32 sq = 0; sq < 64; sq++) {
        u32 n, s;
        int d;
        const u64 key = othu::root_entry<Rules>(t.nodes, legal, sq, n, s, d);
        if (visits) visits[sq] = n, wins[sq] = s, diffs[sq] = d;
        if (key > best) best = key;
    }
    return othu::best_move_of<Rules>(best, P, O);
}

static void print_row(FILE* o, Tree& t) {
    u32 visits[64] = {}, wins[64] = {}, best = othu::kNoMove, root_wins = 0;
    int diffs[64] = {}, root_diffs = 0;
    u64 P = 0, O = 0;
    const bool ok = t.status == OTHR_READY;
    if (ok) {
        t.nodes.pos(0, P, O);
        best = best_move(t, visits, wins, diffs);
        root_wins = 128u * t.nodes.n(0) - t.nodes.ss[0];
        root_diffs = -t.nodes.d(0);
    }
    const bool white = t.turn == 2;
    fprintf(o, "R %u %u %u %u %d %u %llx %llx %u", ok ? OTHR_READY : OTHR_INVALID, best, ok ? t.count : 0u, root_wins,
            root_diffs, t.ran, (unsigned long long)(white ? O : P), (unsigned long long)(white ? P : O), t.turn);
    for (int s = 0; s < 64; s++) fprintf(o, " %u", visits[s]);
    for (int s = 0; s < 64; s++) fprintf(o, " %u", wins[s]);
    for (int s = 0; s < 64; s++) fprintf(o, " %d", diffs[s]);
    fprintf(o, "\n");
}

static void print_dump(FILE* o, Tree& t) {
    const bool ok = t.status == OTHR_READY;
    fprintf(o, "T %u %llu\n", ok ? t.count : 0u, (unsigned long long)t.played);
    if (!ok) return;
    std::vector<u32> order{0};
    for (size_t q = 0; q < order.size(); q++) {
        const u32 v = order[q], link = t.nodes.link(v);
        u64 P, O;
        u32 n, s;
        t.nodes.pos(v, P, O);
        t.nodes.visits_wins(v, n, s);
        fprintf(o, "%llx %llx %u %u %d %u\n", (unsigned long long)P, (unsigned long long)O, n, s, t.nodes.d(v),
                othu::link_cnt(link));
        for (u32 k = 0; k < othu::link_cnt(link); k++) order.push_back(othu::link_first(link) + k);
    }
}

int main(int argc, char** argv) {
    if (argc != 7) usage(argv[0], "IN SCRIPT OUT explore_bits seed max_nodes");
    const u32 cbits = (u32)strtoul(argv[4], nullptr, 16);
    const u64 seed = strtoull(argv[5], nullptr, 0);
    const long M = atol(argv[6]);
    if (M < 1 || M > (long)othu::kMaxNodes) return 2;
    float c;
    memcpy(&c, &cbits, 4);
    std::vector<Pos> starts;  // extra[0]: the tree's id base
    std::vector<float> table;
    read_trees(argv[1], 1, starts, table);
    char line[4096];
    if (table.size() < 2) return 2;
    const size_t n = starts.size();
    std::vector<Tree> trees(n, Tree((u32)M));
    othu::Params p;
    p.iterations = 0;
    p.max_nodes = (u32)M;
    p.explore = c;
    p.log_table = table.data();
    p.seed_state = othp::seed_state(seed);
    p.game_id0 = 0;
    const u32 table_last = (u32)table.size() - 1u;

    FILE* script = fopen(argv[2], "r");
    FILE* o = fopen(argv[3], "w");
    if (!script || !o) return 1;
    HostWave wave;
    while (fgets(line, sizeof line, script)) {
        std::istringstream words(line);
        std::string op;
        if (!(words >> op)) continue;
        if (op == "init") {
            for (size_t i = 0; i < n; i++) {
                Tree& t = trees[i];
                const Pos& s = starts[i];
                const bool white = s.white_to_move(), valid = (s.black & s.white) == 0;
                othu::init_root(t.nodes, wave, s.mover(), s.other());
                t.id_base = s.extra[0], t.played = 0, t.ran = 0;
                t.count = valid ? 1u : 0u;
                t.turn = white ? 2u : 1u;
                t.status = valid ? OTHR_READY : OTHR_INVALID;
            }
        } else if (op == "search") {
            std::vector<u32> counts;
            for (unsigned long long x; words >> x;) counts.push_back((u32)x);
            if (counts.size() != 1 && counts.size() != n) return 2;
            for (size_t i = 0; i < n; i++) {
                Tree& t = trees[i];
                t.ran = 0;
                if (t.status == OTHR_READY) {
                    const u32 want = counts[counts.size() == 1 ? 0 : i], seen = t.nodes.n(0);
                    const u32 room = seen < othu::kMaxIterations ? othu::kMaxIterations - seen : 0u;
                    t.ran = want < room ? want : room;
                    if (t.ran) {
                        t.count = othu::iterate<Rules>(t.nodes, wave, t.id_base, t.played, t.ran, t.count, table_last, p);
                        t.played += t.ran;
                    }
                }
                print_row(o, t);
            }
        } else if (op == "rows") {
            for (size_t i = 0; i < n; i++) {
                trees[i].ran = 0;
                print_row(o, trees[i]);
            }
        } else if (op == "dump") {
            for (size_t i = 0; i < n; i++) print_dump(o, trees[i]);
        } else if (op == "advance") {
            int keep;
            if (!(words >> keep)) return 2;
            std::vector<std::string> how;
            for (std::string x; words >> x;) how.push_back(x);
            if (how.size() != 1 && how.size() != n) return 2;
            for (size_t i = 0; i < n; i++) {
                Tree& t = trees[i];
                const std::string& h = how[how.size() == 1 ? 0 : i];
                u32 move = othu::kNoMove, st = t.status == OTHR_READY ? OTHR_READY : OTHR_INVALID;
                if (st == OTHR_READY) {
                    u64 P, O;
                    t.nodes.pos(0, P, O);
                    if (h == "best") {
                        move = best_move(t, nullptr, nullptr, nullptr);
                    } else if (h == "last") {
                        const u64 legal = Rules::moves(P, O);
                        move = legal ? 63u - (u32)__builtin_clzll(legal) : (Rules::moves(O, P) ? 64u : 255u);
                    } else {
                        move = (u32)strtoul(h.c_str(), nullptr, 0);
                    }
                    if (move != OTHR_KEEP) {
                        if (!othu::may_play<Rules>(P, O, move)) {
                            st = OTHR_BADMOVE;
                        } else {
                            t.count = othu::advance<Rules>(t.nodes, t.half, wave, move, keep != 0, (u32)M);
                            t.turn = 3u - t.turn;
                        }
                    }
                }
                fprintf(o, "A %u %u\n", st, move);
            }
        } else {
            fprintf(stderr, "unknown operation %s\n", op.c_str());
            return 2;
        }
    }
    fclose(script);
    fclose(o);
    return 0;
}
