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
#include "host_io.hpp"
#include "host_rules.hpp"

using othm::u32;
using othm::u64;

using HostStack = HostStack9<othm::kFrames>;

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
    const u64 P = p.mover(), O = p.other();
    othb::begin_search<HostRules>(D, L, P, O, (u32)p.extra[0], cap);
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
    int table[othm::kEvalTable];
    read_weights(argv[4], table);
    std::vector<Pos> pos;
    read_positions(argv[2], 1, pos);
    for (const Pos& p : pos)
        if (p.extra[0] > 0xFFFFFFFFull) return 2;
    std::vector<SearchOut> out(pos.size());
    const long n = (long)pos.size();
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long i = 0; i < n; i++) out[i] = order ? search_one<true>(pos[i], cap, table) : search_one<false>(pos[i], cap, table);
    FILE* o = open_or_exit(argv[3], "w");
    for (const SearchOut& r : out) fprintf(o, "%d %u %u %u %u\n", r.value, r.best, r.status, r.depth, r.nodes);
    fclose(o);
    return 0;
}

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
static void play_one(const Pos& s, u64 key, const othp::Match& m, const othb::Budgets& bud, const int* tables,
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
    FILE* in = open_or_exit(argv[2], "r");
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
    FILE* o = open_or_exit(argv[3], "w");
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
