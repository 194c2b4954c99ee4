// line_host.cpp — the principal variation (subproc_amd/csrc/line_core.hpp around
// solve_core.hpp, search_core.hpp and order_core.hpp) on the host, with a plain
// C++ statement of the rules and OpenMP over positions.
//
// Use, as budget_host.cpp's: the layer's logic can be run under
// -fsanitize=address,undefined and compared against tests/line_ref.py's walk
// over the oracle before any GPU run (the device build differs in the rules
// struct, the stack and the outputs' stores).
//
// build:  g++ -O2 -std=c++17 -fopenmp -o tools/diag/line_host tools/diag/line_host.cpp
// run:    line_host solve IN OUT max_empties [node_limit=0] [threads=16]
//         line_host search IN OUT WEIGHTS depth [order=0] [node_limit=0] [threads=16]
//   IN : one position per line, "<black hex> <white hex> <turn>"; search with
//        depth = -1: "<black hex> <white hex> <turn> <depth>", a depth per position
//   WEIGHTS: 36 integers in -128..127, [phase][feature]
//   OUT: one line per position,
//        "<value> <best_move> <status> <nodes> <length> <end black hex> <end white hex> <end turn> <32 line bytes as hex>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../subproc_amd/csrc/line_core.hpp"
#include "host_io.hpp"
#include "host_rules.hpp"

using othm::u32;
using othm::u64;

struct LineOut {
    int value;
    u32 best, status, nodes, length;
    u64 black, white;
    int end_turn;
    uint8_t row[othl::kLineStride];
    void move(u32 k, u32 code) {
        if (k < (u32)othl::kLineStride) row[k] = (uint8_t)code;
    }
    void clear(u32) { memset(row, 255, sizeof row); }
    void finish(const othl::Walk& W, bool white) {
        const bool white_to_move = white == W.root_side;
        value = W.value;
        best = W.move;
        status = W.status;
        nodes = othl::nodes32(W);
        length = W.len;
        black = white_to_move ? W.O : W.P;
        this->white = white_to_move ? W.P : W.O;
        end_turn = white_to_move ? 2 : 1;
    }
};

static void solve_one(const Pos& p, int max_empties, u32 limit, LineOut& out) {
    out.clear(0);
    const bool white = p.white_to_move();
    const u64 P = p.mover(), O = p.other();
    const u32 st = oths::classify(p.black, p.white, 64 - HostRules::count(p.black | p.white), max_empties);
    othl::Walk W;
    if (st != oths::kSolved) {
        othl::open(W, P, O, 0, st);
        return out.finish(W, white);
    }
    oths::Lane L;
    HostStack7<oths::kFrames> stk;
    othl::begin_solve(W, L, P, O);
    do {
        while (L.depth >= 0) oths::advance<HostRules>(L, stk, limit);
    } while (othl::follow_solve<HostRules>(W, L, out));
    out.finish(W, white);
}

template <bool kOrdered>
static void search_one(const Pos& p, u32 depth, const int* table, u32 limit, LineOut& out) {
    out.clear(0);
    const bool white = p.white_to_move();
    const u64 P = p.mover(), O = p.other();
    const u32 st = (p.black & p.white) ? othm::kInvalid : othl::classify_depth(depth);
    othl::Walk W;
    if (st != othm::kSearched) {
        othl::open(W, P, O, 0, st);
        return out.finish(W, white);
    }
    othm::Lane L;
    HostStack9<othm::kFrames> stk;
    othm::Order Q;
    othl::begin_search(W, L, P, O, (int)depth);
    do {
        othm::order_reset(Q);
        while (L.depth >= 0) {
            if constexpr (kOrdered)
                othm::advance_ordered<HostRules, true>(L, Q, stk, table, limit);
            else
                othm::advance<HostRules>(L, stk, table, limit);
        }
    } while (othl::follow_search<HostRules>(W, L, out));
    out.finish(W, white);
}

static int write_out(const char* path, const std::vector<LineOut>& out) {
    FILE* o = open_or_exit(path, "w");
    for (const LineOut& r : out) {
        fprintf(o, "%d %u %u %u %u %llx %llx %d ", r.value, r.best, r.status, r.nodes, r.length,
                (unsigned long long)r.black, (unsigned long long)r.white, r.end_turn);
        for (int k = 0; k < othl::kLineStride; k++) fprintf(o, "%02x", r.row[k]);
        fprintf(o, "\n");
    }
    fclose(o);
    return 0;
}

static int main_solve(int argc, char** argv) {
    if (argc < 5) return 2;
    const int max_empties = atoi(argv[4]);
    const unsigned long long limit_arg = argc > 5 ? strtoull(argv[5], nullptr, 10) : 0;
    const int threads = argc > 6 ? atoi(argv[6]) : 16;
    if (max_empties < 0 || max_empties > oths::kMaxEmpties || limit_arg > 0xFFFFFFFFull || threads < 1) return 2;
    const u32 limit = node_limit(limit_arg);
    std::vector<Pos> pos;
    read_positions(argv[2], 0, pos);
    std::vector<LineOut> out(pos.size());
    const long n = (long)pos.size();
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long i = 0; i < n; i++) solve_one(pos[(size_t)i], max_empties, limit, out[(size_t)i]);
    return write_out(argv[3], out);
}

static int main_search(int argc, char** argv) {
    if (argc < 6) return 2;
    const int depth = atoi(argv[5]);
    const int order = argc > 6 ? atoi(argv[6]) : 0;
    const unsigned long long limit_arg = argc > 7 ? strtoull(argv[7], nullptr, 10) : 0;
    const int threads = argc > 8 ? atoi(argv[8]) : 16;
    if ((depth != -1 && (depth < 1 || depth > othm::kMaxDepth)) || order < 0 || order > 1 ||
        limit_arg > 0xFFFFFFFFull || threads < 1)
        return 2;
    const u32 limit = node_limit(limit_arg);
    int table[othm::kEvalTable];
    read_weights(argv[4], table);
    std::vector<Pos> pos;
    if (read_positions(argv[2], depth == -1, pos) == 3) return 1;  // a line without its depth
    std::vector<LineOut> out(pos.size());
    const long n = (long)pos.size();
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long i = 0; i < n; i++) {
        const Pos& p = pos[(size_t)i];
        const u32 d = depth == -1 ? (u32)p.extra[0] : (u32)depth;
        if (order)
            search_one<true>(p, d, table, limit, out[(size_t)i]);
        else
            search_one<false>(p, d, table, limit, out[(size_t)i]);
    }
    return write_out(argv[3], out);
}

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "solve") == 0) return main_solve(argc, argv);
    if (argc >= 2 && strcmp(argv[1], "search") == 0) return main_search(argc, argv);
    fprintf(stderr,
            "usage: %s solve IN OUT max_empties [node_limit] [threads]\n"
            "       %s search IN OUT WEIGHTS depth|-1 [order] [node_limit] [threads]\n",
            argv[0], argv[0]);
    return 2;
}
