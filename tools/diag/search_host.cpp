// search_host.cpp — the depth-limited search's state machine
// (subproc_amd/csrc/search_core.hpp) on the host, with a plain C++ statement of
// the rules and OpenMP over positions.
//
// Two uses, as solve_host.cpp's:
//   * the search's logic can be run under -fsanitize=address,undefined and
//     compared against tests/search_ref.py's exhaustive minimax before any GPU
//     run (the device build differs in the rules struct and the stack only);
//   * the CPU context line of tools/search_bench.py (16 threads).
//
// build:  g++ -O2 -std=c++17 -fopenmp -o search_host tools/diag/search_host.cpp
// run:    search_host IN OUT WEIGHTS depth [node_limit=0] [threads=16] [order=0]
//   order 1: order_core.hpp's ordered machine (include/othello_order.h)
//   IN : one position per line, "<black hex> <white hex> <turn>"
//   WEIGHTS: 36 integers in -128..127, [phase][feature]
//   OUT: one line per position, "<value> <best_move> <status> <nodes>"
//   stderr: one JSON line with the wall time
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../subproc_amd/csrc/order_core.hpp"
#include "../../subproc_amd/csrc/search_core.hpp"
#include "host_io.hpp"
#include "host_rules.hpp"

using othm::u32;
using othm::u64;

using HostStack = HostStack9<othm::kFrames>;

struct Out {
    int value;
    u32 best, status, nodes;
};

static Out search_one(const Pos& p, int depth, const int* table, u32 limit, int order) {
    if (p.black & p.white) return Out{0, othm::kNoMove, othm::kInvalid, 0};
    othm::Lane L;
    HostStack stk;
    othm::start(L, p.mover(), p.other(), depth);
    othm::Order Q;
    othm::order_reset(Q);
    if (order)
        while (L.depth >= 0) othm::advance_ordered<HostRules, true>(L, Q, stk, table, limit);
    else
        while (L.depth >= 0) othm::advance<HostRules>(L, stk, table, limit);
    return Out{L.value, L.best_mv, L.status, L.nodes};
}

int main(int argc, char** argv) {
    if (argc < 5) usage(argv[0], "IN OUT WEIGHTS depth [node_limit] [threads] [order]");
    const int depth = atoi(argv[4]);
    const u32 limit_arg = argc > 5 ? (u32)strtoul(argv[5], nullptr, 0) : 0u;
    const int threads = argc > 6 ? atoi(argv[6]) : 16;
    const int order = argc > 7 ? atoi(argv[7]) : 0;
    if (depth < 1 || depth > othm::kMaxDepth || threads < 1 || order < 0 || order > 1) return 2;
    const u32 limit = node_limit(limit_arg);
    int table[othm::kEvalTable];
    read_weights(argv[3], table);
    std::vector<Pos> pos;
    read_positions(argv[1], 0, pos);
    std::vector<Out> out(pos.size());
    const auto t0 = std::chrono::steady_clock::now();
    const long n = (long)pos.size();
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long i = 0; i < n; i++) out[i] = search_one(pos[i], depth, table, limit, order);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    FILE* o = open_or_exit(argv[2], "w");
    unsigned long long nodes = 0;
    for (const Out& r : out) {
        fprintf(o, "%d %u %u %u\n", r.value, r.best, r.status, r.nodes);
        nodes += r.nodes;
    }
    fclose(o);
    fprintf(stderr,
            "{\"positions\": %ld, \"threads\": %d, \"depth\": %d, \"order\": %d, \"seconds\": %.6f, \"positions_per_s\": %.1f, "
            "\"nodes\": %llu}\n",
            n, threads, depth, order, sec, sec > 0 ? n / sec : 0.0, nodes);
    return 0;
}
