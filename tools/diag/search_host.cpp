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

using othm::u32;
using othm::u64;

struct HostRules {
    static constexpr int dx[8] = {1, -1, 0, 0, 1, -1, -1, 1};
    static constexpr int dy[8] = {0, 0, 1, -1, 1, -1, 1, -1};
    static int count(u64 x) { return __builtin_popcountll(x); }
    static u32 lowest(u64 m) { return (u32)__builtin_ctzll(m); }
    static int mul(int w, int c) { return w * c; }
    // the opponent discs the move on empty square sq turns over
    static u64 flips(u32 sq, u64 P, u64 O) {
        u64 all = 0;
        for (int d = 0; d < 8; d++) {
            int x = (int)(sq & 7) + dx[d], y = (int)(sq >> 3) + dy[d];
            u64 run = 0;
            while (x >= 0 && x < 8 && y >= 0 && y < 8 && (O >> (x + 8 * y) & 1)) {
                run |= 1ull << (x + 8 * y);
                x += dx[d];
                y += dy[d];
            }
            if (run && x >= 0 && x < 8 && y >= 0 && y < 8 && (P >> (x + 8 * y) & 1)) all |= run;
        }
        return all;
    }
    static u64 moves(u64 P, u64 O) {
        u64 m = 0;
        for (u64 e = ~(P | O); e; e &= e - 1) {
            const u32 sq = lowest(e);
            if (flips(sq, P, O)) m |= 1ull << sq;
        }
        return m;
    }
};

struct HostStack {
    u64 P[othm::kFrames], O[othm::kFrames], M[othm::kFrames];
    int a[othm::kFrames], b[othm::kFrames];
    u32 w[othm::kFrames];
    void store(int d, u64 p, u64 o, u64 m, int al, int be, u32 ww) {
        P[d] = p, O[d] = o, M[d] = m, a[d] = al, b[d] = be, w[d] = ww;
    }
    void load(int d, u64& p, u64& o, u64& m, int& al, int& be, u32& ww) const {
        p = P[d], o = O[d], m = M[d], al = a[d], be = b[d], ww = w[d];
    }
};

struct Pos {
    u64 black, white;
    int turn;
};
struct Out {
    int value;
    u32 best, status, nodes;
};

static Out search_one(const Pos& p, int depth, const int* table, u32 limit, int order) {
    if (p.black & p.white) return Out{0, othm::kNoMove, othm::kInvalid, 0};
    othm::Lane L;
    HostStack stk;
    const bool white = p.turn == 2;
    othm::start(L, white ? p.white : p.black, white ? p.black : p.white, depth);
    othm::Order Q;
    othm::order_reset(Q);
    if (order)
        while (L.depth >= 0) othm::advance_ordered<HostRules, true>(L, Q, stk, table, limit);
    else
        while (L.depth >= 0) othm::advance<HostRules>(L, stk, table, limit);
    return Out{L.value, L.best_mv, L.status, L.nodes};
}

int main(int argc, char** argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: %s IN OUT WEIGHTS depth [node_limit] [threads] [order]\n", argv[0]);
        return 2;
    }
    const int depth = atoi(argv[4]);
    const u32 limit_arg = argc > 5 ? (u32)strtoul(argv[5], nullptr, 0) : 0u;
    const int threads = argc > 6 ? atoi(argv[6]) : 16;
    const int order = argc > 7 ? atoi(argv[7]) : 0;
    if (depth < 1 || depth > othm::kMaxDepth || threads < 1 || order < 0 || order > 1) return 2;
    const u32 limit = limit_arg ? limit_arg : (1u << 28);
    FILE* wf = fopen(argv[3], "r");
    if (!wf) return 1;
    int8_t w36[othm::kEvalPhases * othm::kEvalFeatures];
    for (int8_t& w : w36) {
        int v;
        if (fscanf(wf, "%d", &v) != 1 || v < -128 || v > 127) return 2;
        w = (int8_t)v;
    }
    fclose(wf);
    int table[othm::kEvalTable];
    for (int e = 0; e < othm::kEvalTable; e++) othm::widen_weight(w36, e, table);
    FILE* in = fopen(argv[1], "r");
    if (!in) return 1;
    std::vector<Pos> pos;
    unsigned long long b, w;
    int t;
    while (fscanf(in, "%llx %llx %d", &b, &w, &t) == 3) pos.push_back(Pos{b, w, t});
    fclose(in);
    std::vector<Out> out(pos.size());
    const auto t0 = std::chrono::steady_clock::now();
    const long n = (long)pos.size();
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long i = 0; i < n; i++) out[i] = search_one(pos[i], depth, table, limit, order);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    FILE* o = fopen(argv[2], "w");
    if (!o) return 1;
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
