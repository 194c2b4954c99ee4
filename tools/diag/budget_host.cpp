// budget_host.cpp — the searches by node budget
// (subproc_amd/csrc/budget_core.hpp around search_core.hpp, order_core.hpp and
// play_core.hpp) on the host, with a plain C++ statement of the rules and OpenMP
// over positions / games.
//
// Use, as search_host.cpp's and play_host.cpp's: the deepening layer's logic can
// be run under -fsanitize=address,undefined and compared against
// tests/budget_ref.py's loop before any GPU run (the device build differs in the
// rules struct, the stack and the outputs' stores).
//
// build:  g++ -O2 -std=c++17 -fopenmp -o tools/diag/budget_host tools/diag/budget_host.cpp
// run:    budget_host search IN OUT WEIGHTS max_depth [order=0] [threads=16]
//   IN : one position per line, "<black hex> <white hex> <turn> <budget>"
//   WEIGHTS: 36 integers in -128..127, [phase][feature]
//   OUT: one line per position, "<value> <best_move> <status> <depth> <nodes>"
// run:    budget_host play ARGS OUT [order=0] [threads=16]
//   ARGS: play_host.cpp's file with the budgets after the depths,
//           line 1: n seed game_id0 depth_a depth_b budget_a budget_b exact_empties n_rand_a n_rand_b swap
//                   node_limit have_start
//           line 2: A's 36 weights, line 3: B's 36 weights
//           then, with have_start != 0, n lines "<black hex> <white hex> <turn>"
//   OUT:  play_host.cpp's: "<a_black> <black hex> <white hex> <diff> <plies> <status> <nodes> <128 move bytes as hex>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../subproc_amd/csrc/budget_core.hpp"
#include "host_rules.hpp"

using othm::u32;
using othm::u64;

using HostStack = HostStack9<othm::kFrames>;

static bool read_weights(FILE* f, int8_t* w36) {
    for (int k = 0; k < othm::kEvalPhases * othm::kEvalFeatures; k++) {
        int v;
        if (fscanf(f, "%d", &v) != 1 || v < -128 || v > 127) return false;
        w36[k] = (int8_t)v;
    }
    return true;
}

struct Pos {
    u64 black, white;
    int turn;
    u32 budget;
};
struct SearchOut {
    int value;
    u32 best, status, depth, nodes;
};

template <bool kOrdered>
static SearchOut search_one(const Pos& p, int cap, const int* table) {
    if (p.black & p.white) return SearchOut{0, othm::kNoMove, othm::kInvalid, 0, 0};
    othm::Lane L;
    HostStack stk;
    othm::Order Q;
    othm::order_reset(Q);
    othb::Deepen D{};
    const bool white = p.turn == 2;
    const u64 P = white ? p.white : p.black, O = white ? p.black : p.white;
    othb::begin_search<HostRules>(D, L, P, O, p.budget, cap);
    if (L.depth >= 0)
        while (!othb::advance_search<HostRules, kOrdered>(D, L, Q, stk, table, P, O)) {
        }
    return SearchOut{D.value, D.move, othb::status_of(D), D.depth, D.nodes};
}

static int main_search(int argc, char** argv) {
    if (argc < 6) return 2;
    const int cap = atoi(argv[5]);
    const int order = argc > 6 ? atoi(argv[6]) : 0;
    const int threads = argc > 7 ? atoi(argv[7]) : 16;
    if (cap < 1 || cap > othm::kMaxDepth || threads < 1 || order < 0 || order > 1) return 2;
    FILE* wf = fopen(argv[4], "r");
    if (!wf) return 1;
    int8_t w36[othm::kEvalPhases * othm::kEvalFeatures];
    if (!read_weights(wf, w36)) return 2;
    fclose(wf);
    int table[othm::kEvalTable];
    for (int e = 0; e < othm::kEvalTable; e++) othm::widen_weight(w36, e, table);
    FILE* in = fopen(argv[2], "r");
    if (!in) return 1;
    std::vector<Pos> pos;
    unsigned long long b, w, budget;
    int t;
    while (fscanf(in, "%llx %llx %d %llu", &b, &w, &t, &budget) == 4) {
        if (budget > 0xFFFFFFFFull) return 2;
        pos.push_back(Pos{b, w, t, (u32)budget});
    }
    fclose(in);
    std::vector<SearchOut> out(pos.size());
    const long n = (long)pos.size();
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long i = 0; i < n; i++) out[i] = order ? search_one<true>(pos[i], cap, table) : search_one<false>(pos[i], cap, table);
    FILE* o = fopen(argv[3], "w");
    if (!o) return 1;
    for (const SearchOut& r : out) fprintf(o, "%d %u %u %u %u\n", r.value, r.best, r.status, r.depth, r.nodes);
    fclose(o);
    return 0;
}

struct Start {
    u64 black, white;
    int turn;
};
struct GameOut {
    int a_black, diff;
    u64 black, white, nodes;
    u32 plies, status;
    uint8_t moves[othp::kMovesStride];
    void move(u32 ply, u32 code) {
        if (ply < othp::kMovesStride) moves[ply] = (uint8_t)code;
    }
};

template <bool kOrdered>
static void play_one(const Start& s, u64 key, const othp::Match& m, const othb::Budgets& bud, const int* tables,
                     GameOut& out) {
    memset(out.moves, 255, sizeof out.moves);
    othp::Game G;
    othm::Lane L;
    HostStack stk;
    othm::Order Q;
    othm::order_reset(Q);
    othb::Deepen D{};
    D.d = 0;
    othp::begin(G, L, m, key, s.black, s.white, s.turn == 2);
    while (G.live) othb::advance_play<HostRules, kOrdered>(G, L, Q, D, stk, tables, m, bud, out);
    out.a_black = G.a_black;
    out.black = othp::black_of(G);
    out.white = othp::white_of(G);
    out.diff = G.status == othm::kInvalid ? 0 : HostRules::count(out.black) - HostRules::count(out.white);
    out.plies = G.ply;
    out.status = G.status;
    out.nodes = G.nodes;
}

static int main_play(int argc, char** argv) {
    if (argc < 4) return 2;
    const int order = argc > 4 ? atoi(argv[4]) : 0;
    const int threads = argc > 5 ? atoi(argv[5]) : 16;
    if (threads < 1 || order < 0 || order > 1) return 2;
    FILE* in = fopen(argv[2], "r");
    if (!in) return 1;
    long n;
    unsigned long long seed, id0, limit_arg, ba, bb;
    int da, db, exact, ra, rb, swap, have_start;
    if (fscanf(in, "%ld %llu %llu %d %d %llu %llu %d %d %d %d %llu %d", &n, &seed, &id0, &da, &db, &ba, &bb, &exact, &ra,
               &rb, &swap, &limit_arg, &have_start) != 13)
        return 2;
    if (n < 0 || da < 1 || da > othm::kMaxDepth || db < 1 || db > othm::kMaxDepth || exact < 0 ||
        exact > othm::kMaxDepth || ra < 0 || rb < 0 || limit_arg > 0xFFFFFFFFull || ba < 1 || ba > 0xFFFFFFFFull ||
        bb < 1 || bb > 0xFFFFFFFFull)
        return 2;
    int8_t w36[2][othm::kEvalPhases * othm::kEvalFeatures];
    if (!read_weights(in, w36[0]) || !read_weights(in, w36[1])) return 2;
    int tables[2 * othm::kEvalTable];
    for (int p = 0; p < 2; p++)
        for (int e = 0; e < othm::kEvalTable; e++) othm::widen_weight(w36[p], e, tables + p * othm::kEvalTable);
    std::vector<Start> starts((size_t)n, Start{othp::kOpenBlack, othp::kOpenWhite, 1});
    if (have_start)
        for (long i = 0; i < n; i++) {
            unsigned long long b, w;
            int t;
            if (fscanf(in, "%llx %llx %d", &b, &w, &t) != 3) return 2;
            starts[(size_t)i] = Start{b, w, t};
        }
    fclose(in);
    othp::Match m;
    m.depth[0] = da;
    m.depth[1] = db;
    m.n_rand[0] = (u32)(ra < (int)othp::kMaxBudget ? ra : (int)othp::kMaxBudget);
    m.n_rand[1] = (u32)(rb < (int)othp::kMaxBudget ? rb : (int)othp::kMaxBudget);
    m.exact_empties = exact;
    m.limit = limit_arg ? (u32)limit_arg : (1u << 28);
    m.swap = swap != 0;
    othb::Budgets bud;
    bud.budget[0] = (u32)ba;
    bud.budget[1] = (u32)bb;
    const u64 S = othp::seed_state(seed);
    std::vector<GameOut> out((size_t)n);
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long i = 0; i < n; i++) {
        const u64 key = othp::game_key(S, id0 + (u64)i);
        if (order)
            play_one<true>(starts[(size_t)i], key, m, bud, tables, out[(size_t)i]);
        else
            play_one<false>(starts[(size_t)i], key, m, bud, tables, out[(size_t)i]);
    }
    FILE* o = fopen(argv[3], "w");
    if (!o) return 1;
    for (const GameOut& r : out) {
        fprintf(o, "%d %llx %llx %d %u %u %llu ", r.a_black, (unsigned long long)r.black, (unsigned long long)r.white,
                r.diff, r.plies, r.status, (unsigned long long)r.nodes);
        for (u32 k = 0; k < othp::kMovesStride; k++) fprintf(o, "%02x", r.moves[k]);
        fprintf(o, "\n");
    }
    fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "search") == 0) return main_search(argc, argv);
    if (argc >= 2 && strcmp(argv[1], "play") == 0) return main_play(argc, argv);
    fprintf(stderr, "usage: %s search IN OUT WEIGHTS max_depth [order] [threads]\n       %s play ARGS OUT [order] [threads]\n",
            argv[0], argv[0]);
    return 2;
}
