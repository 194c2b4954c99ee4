// solve_host.cpp — the endgame solver's state machine (subproc_amd/csrc/solve_core.hpp)
// on the host, with a plain C++ statement of the rules and OpenMP over positions.
//
// Two uses:
//   * the solver's logic can be run under -fsanitize=address,undefined and
//     compared against tests/solve_ref.py's exhaustive minimax before any GPU
//     run (the device build differs in the rules struct and the stack only);
//   * the CPU context line of tools/solve_bench.py (16 threads).
//
// build:  g++ -O2 -std=c++17 -fopenmp -o solve_host tools/diag/solve_host.cpp
// run:    solve_host IN OUT [max_empties=12] [node_limit=0] [threads=16]
//   IN : one position per line, "<black hex> <white hex> <turn>"
//   OUT: one line per position, "<value> <best_move> <status> <nodes>"
//   stderr: one JSON line with the wall time
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../subproc_amd/csrc/solve_core.hpp"
#include "host_io.hpp"
#include "host_rules.hpp"

using oths::u32;
using oths::u64;

using HostStack = HostStack7<oths::kFrames>;

struct Out {
    int value;
    u32 best, status, nodes;
};

static Out solve_one(const Pos& p, int max_empties, u32 limit) {
    const u32 st = oths::classify(p.black, p.white, 64 - HostRules::count(p.black | p.white), max_empties);
    if (st != oths::kSolved) return Out{0, oths::kNoMove, st, 0};
    oths::Lane L;
    HostStack stk;
    oths::start(L, p.mover(), p.other());
    while (L.depth >= 0) oths::advance<HostRules>(L, stk, limit);
    return Out{L.value, L.best_mv, L.status, L.nodes};
}

int main(int argc, char** argv) {
    if (argc < 3) usage(argv[0], "IN OUT [max_empties] [node_limit] [threads]");
    const int max_empties = argc > 3 ? atoi(argv[3]) : oths::kMaxEmpties;
    const u32 limit_arg = argc > 4 ? (u32)strtoul(argv[4], nullptr, 0) : 0u;
    const int threads = argc > 5 ? atoi(argv[5]) : 16;
    if (max_empties < 0 || max_empties > oths::kMaxEmpties || threads < 1) return 2;
    const u32 limit = node_limit(limit_arg);
    std::vector<Pos> pos;
    read_positions(argv[1], 0, pos);
    std::vector<Out> out(pos.size());
    const auto t0 = std::chrono::steady_clock::now();
    const long n = (long)pos.size();
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long i = 0; i < n; i++) out[i] = solve_one(pos[i], max_empties, limit);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    FILE* o = open_or_exit(argv[2], "w");
    unsigned long long nodes = 0;
    for (const Out& r : out) {
        fprintf(o, "%d %u %u %u\n", r.value, r.best, r.status, r.nodes);
        nodes += r.nodes;
    }
    fclose(o);
    fprintf(stderr, "{\"positions\": %ld, \"threads\": %d, \"seconds\": %.6f, \"positions_per_s\": %.1f, \"nodes\": %llu}\n",
            n, threads, sec, sec > 0 ? n / sec : 0.0, nodes);
    return 0;
}
