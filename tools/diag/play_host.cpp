// play_host.cpp — the search self-play's game driver
// (subproc_amd/csrc/play_core.hpp around search_core.hpp) on the host, with a
// plain C++ statement of the rules and OpenMP over games.
//
// Two uses, as search_host.cpp's:
//   * the driver's logic can be run under -fsanitize=address,undefined and
//     compared against tests/play_ref.py's games before any GPU run (the device
//     build differs in the rules struct, the stack and the outputs' stores);
//   * the CPU context line of tools/play_bench.py (16 threads).
//
// build:  g++ -O2 -std=c++17 -fopenmp -o tools/diag/play_host tools/diag/play_host.cpp
// run:    play_host ARGS OUT [threads=16] [order=0]
//   order 1: order_core.hpp's ordered machine in every search (include/othello_order.h)
//   ARGS: a text file,
//           line 1: n seed game_id0 depth_a depth_b exact_empties n_rand_a n_rand_b swap node_limit have_start
//           line 2: A's 36 weights, line 3: B's 36 weights (integers -128..127)
//           then, with have_start != 0, n lines "<black hex> <white hex> <turn>"
//   OUT:  one line per game,
//           "<a_black> <black hex> <white hex> <diff> <plies> <status> <nodes> <128 move bytes as hex>"
//   stderr: one JSON line with the wall time
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../subproc_amd/csrc/play_core.hpp"
#include "host_io.hpp"
#include "host_rules.hpp"

using othm::u32;
using othm::u64;

using HostStack = HostStack9<othm::kFrames>;

struct Out {
    int a_black, diff;
    u64 black, white, nodes;
    u32 plies, status;
    uint8_t moves[othp::kMovesStride];
    void move(u32 ply, u32 code) {
        if (ply < othp::kMovesStride) moves[ply] = (uint8_t)code;
    }
};

static void play_one(const Pos& s, u64 key, const othp::Match& m, const int* tables, int order, Out& out) {
    memset(out.moves, 255, sizeof out.moves);
    othp::Game G;
    othm::Lane L;
    HostStack stk;
    othp::begin(G, L, m, key, s.black, s.white, s.turn == 2);
    othm::Order Q;
    othm::order_reset(Q);
    if (order)
        while (G.live) othp::advance<HostRules, true>(G, L, Q, stk, tables, m, out);
    else
        while (G.live) othp::advance<HostRules, false>(G, L, Q, stk, tables, m, out);
    out.a_black = G.a_black;
    out.black = othp::black_of(G);
    out.white = othp::white_of(G);
    out.diff = G.status == othm::kInvalid ? 0 : HostRules::count(out.black) - HostRules::count(out.white);
    out.plies = G.ply;
    out.status = G.status;
    out.nodes = G.nodes;
}

int main(int argc, char** argv) {
    if (argc < 3) usage(argv[0], "ARGS OUT [threads] [order]");
    const int threads = argc > 3 ? atoi(argv[3]) : 16;
    const int order = argc > 4 ? atoi(argv[4]) : 0;
    if (threads < 1 || order < 0 || order > 1) return 2;
    FILE* in = open_or_exit(argv[1], "r");
    long n;
    unsigned long long seed, id0, limit_arg;
    int da, db, exact, ra, rb, swap, have_start;
    if (fscanf(in, "%ld %llu %llu %d %d %d %d %d %d %llu %d", &n, &seed, &id0, &da, &db, &exact, &ra, &rb, &swap,
               &limit_arg, &have_start) != 11)
        return 2;
    if (n < 0 || da < 1 || da > othm::kMaxDepth || db < 1 || db > othm::kMaxDepth || exact < 0 ||
        exact > othm::kMaxDepth || ra < 0 || rb < 0 || limit_arg > 0xFFFFFFFFull)
        return 2;
    int tables[2 * othm::kEvalTable];
    if (!read_weights(in, tables) || !read_weights(in, tables + othm::kEvalTable)) return 2;
    std::vector<Pos> starts;
    if (have_start) {
        read_positions(in, 0, starts, n);
        if ((long)starts.size() != n) return 2;
    } else {
        starts.assign((size_t)n, Pos{othp::kOpenBlack, othp::kOpenWhite, 1, {0, 0}});
    }
    fclose(in);
    othp::Match m;
    m.depth[0] = da;
    m.depth[1] = db;
    m.n_rand[0] = (u32)(ra < (int)othp::kMaxBudget ? ra : (int)othp::kMaxBudget);
    m.n_rand[1] = (u32)(rb < (int)othp::kMaxBudget ? rb : (int)othp::kMaxBudget);
    m.exact_empties = exact;
    m.limit = node_limit(limit_arg);
    m.swap = swap != 0;
    const u64 S = othp::seed_state(seed);
    std::vector<Out> out((size_t)n);
    const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long i = 0; i < n; i++) play_one(starts[(size_t)i], othp::game_key(S, id0 + (u64)i), m, tables, order, out[(size_t)i]);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    FILE* o = open_or_exit(argv[2], "w");
    unsigned long long nodes = 0, plies = 0;
    for (const Out& r : out) {
        fprintf(o, "%d %llx %llx %d %u %u %llu ", r.a_black, (unsigned long long)r.black, (unsigned long long)r.white,
                r.diff, r.plies, r.status, (unsigned long long)r.nodes);
        for (u32 k = 0; k < othp::kMovesStride; k++) fprintf(o, "%02x", r.moves[k]);
        fprintf(o, "\n");
        nodes += r.nodes;
        plies += r.plies;
    }
    fclose(o);
    fprintf(stderr,
            "{\"games\": %ld, \"threads\": %d, \"depth_a\": %d, \"depth_b\": %d, \"order\": %d, \"seconds\": %.6f, "
            "\"games_per_s\": %.1f, \"plies\": %llu, \"nodes\": %llu}\n",
            n, threads, da, db, order, sec, sec > 0 ? n / sec : 0.0, plies, nodes);
    return 0;
}
