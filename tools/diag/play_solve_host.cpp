// play_solve_host.cpp — search self-play whose last plies are the exact
// solver's (subproc_amd/csrc/play_solve_core.hpp around play_core.hpp,
// budget_core.hpp and solve_core.hpp) on the host, with a plain C++ statement of
// the rules.  Both phases of play_solve.hip run here over the same cores: the
// first parks the games that reach the zone into a list of records, the second
// takes the list up and plays each game to its end with the solver.
//
// Use, as play_host.cpp's and budget_host.cpp's: the two phases' logic can be
// run under -fsanitize=address,undefined and compared against
// tests/play_ref.py's games before any GPU run (the device build differs in the
// rules struct, the stacks, the list's atomics and the outputs' stores).
//
// build:  g++ -O2 -std=c++17 -fopenmp -o tools/diag/play_solve_host tools/diag/play_solve_host.cpp
// run:    play_solve_host ARGS OUT [order=0] [threads=16]
//   ARGS: budget_host.cpp's file for its games, with solve_empties where exact_empties stands and 0 0 for
//         "no budgets: fixed depth",
//           line 1: n seed game_id0 depth_a depth_b budget_a budget_b solve_empties n_rand_a n_rand_b swap
//                   node_limit have_start
//           line 2: A's 36 weights, line 3: B's 36 weights
//           then, with have_start != 0, n lines "<black hex> <white hex> <turn>"
//   OUT:  play_host.cpp's: "<a_black> <black hex> <white hex> <diff> <plies> <status> <nodes> <128 move bytes as hex>"
//   stderr: one line, "parked <count> of <n>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../subproc_amd/csrc/budget_core.hpp"
#include "../../subproc_amd/csrc/play_solve_core.hpp"
#include "host_io.hpp"
#include "host_rules.hpp"

using othm::u32;
using othm::u64;

using SearchStack = HostStack9<othm::kFrames>;
using SolveStack = HostStack7<oths::kFrames>;

struct GameOut {
    int a_black, diff;
    u64 black, white, nodes;
    u32 plies, status;
    uint8_t moves[othp::kMovesStride];
    void move(u32 ply, u32 code) {
        if (ply < othp::kMovesStride) moves[ply] = (uint8_t)code;
    }
};
struct Record {
    u64 w[othx::kRecordWords];
};

static void emit(const othp::Game& G, GameOut& out) {
    out.a_black = G.a_black;
    out.black = othp::black_of(G);
    out.white = othp::white_of(G);
    out.diff = G.status == othm::kInvalid ? 0 : HostRules::count(out.black) - HostRules::count(out.white);
    out.plies = G.ply;
    out.status = G.status;
    out.nodes = G.nodes;
}

// the first phase of game g: true = parked into `rec`, false = ended and emitted
template <bool kOrdered, bool kBudget>
static bool first_phase(const Pos& s, u64 key, u64 g, const othp::Match& m, const othb::Budgets& bud,
                        const int* tables, GameOut& out, Record& rec) {
    memset(out.moves, 255, sizeof out.moves);
    othp::Game G;
    othm::Lane L;
    SearchStack stk;
    othm::Order Q;
    othm::order_reset(Q);
    othb::Deepen D{};
    D.d = 0;
    othp::begin(G, L, m, key, s.black, s.white, s.turn == 2);
    while (G.live) {
        if constexpr (kBudget)
            othb::advance_play<HostRules, kOrdered, true>(G, L, Q, D, stk, tables, m, bud, out);
        else
            othp::advance<HostRules, kOrdered, true>(G, L, Q, stk, tables, m, out);
    }
    if (G.status == othp::kParked) {
        othx::pack(G, g, rec.w);
        return true;
    }
    emit(G, out);
    return false;
}

static void second_phase(const Record& rec, u32 limit, std::vector<GameOut>& outs) {
    othp::Game G;
    oths::Lane L;
    L.depth = -1;
    SolveStack stk;
    const u64 g = othx::unpack(G, rec.w);
    GameOut& out = outs[(size_t)g];
    while (G.live) othx::advance<HostRules>(G, L, stk, limit, out);
    emit(G, out);
}

int main(int argc, char** argv) {
    if (argc < 3) usage(argv[0], "ARGS OUT [order] [threads]");
    const int order = argc > 3 ? atoi(argv[3]) : 0;
    const int threads = argc > 4 ? atoi(argv[4]) : 16;
    if (threads < 1 || order < 0 || order > 1) return 2;
    FILE* in = open_or_exit(argv[1], "r");
    long n;
    unsigned long long seed, id0, limit_arg, ba, bb;
    int da, db, zone, ra, rb, swap, have_start;
    if (fscanf(in, "%ld %llu %llu %d %d %llu %llu %d %d %d %d %llu %d", &n, &seed, &id0, &da, &db, &ba, &bb, &zone, &ra,
               &rb, &swap, &limit_arg, &have_start) != 13)
        return 2;
    if (n < 0 || da < 1 || da > othm::kMaxDepth || db < 1 || db > othm::kMaxDepth || zone < 1 ||
        zone > oths::kMaxEmpties || ra < 0 || rb < 0 || limit_arg > 0xFFFFFFFFull || ba > 0xFFFFFFFFull ||
        bb > 0xFFFFFFFFull || (ba == 0) != (bb == 0))
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
    m.exact_empties = zone;  // the first phase's parking line
    m.limit = node_limit(limit_arg);
    m.swap = swap != 0;
    othb::Budgets bud;
    bud.budget[0] = (u32)ba;
    bud.budget[1] = (u32)bb;
    const bool budgeted = ba != 0;
    const u64 S = othp::seed_state(seed);
    std::vector<GameOut> out((size_t)n);
    std::vector<Record> slot((size_t)n);
    std::vector<uint8_t> is_parked((size_t)n, 0);
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long i = 0; i < n; i++) {
        const u64 key = othp::game_key(S, id0 + (u64)i);
        const Pos& s = starts[(size_t)i];
        GameOut& o = out[(size_t)i];
        Record& r = slot[(size_t)i];
        bool p;
        if (budgeted)
            p = order ? first_phase<true, true>(s, key, (u64)i, m, bud, tables, o, r)
                      : first_phase<false, true>(s, key, (u64)i, m, bud, tables, o, r);
        else
            p = order ? first_phase<true, false>(s, key, (u64)i, m, bud, tables, o, r)
                      : first_phase<false, false>(s, key, (u64)i, m, bud, tables, o, r);
        is_parked[(size_t)i] = p;
    }
    // the list, compacted (in game order here; the device's order is the lanes' arrival, and nothing reads it)
    std::vector<Record> list;
    for (long i = 0; i < n; i++)
        if (is_parked[(size_t)i]) list.push_back(slot[(size_t)i]);
    const long parked = (long)list.size();
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long k = 0; k < parked; k++) second_phase(list[(size_t)k], m.limit, out);
    fprintf(stderr, "parked %ld of %ld\n", parked, n);
    FILE* o = open_or_exit(argv[2], "w");
    for (const GameOut& r : out) {
        fprintf(o, "%d %llx %llx %d %u %u %llu ", r.a_black, (unsigned long long)r.black, (unsigned long long)r.white,
                r.diff, r.plies, r.status, (unsigned long long)r.nodes);
        for (u32 k = 0; k < othp::kMovesStride; k++) fprintf(o, "%02x", r.moves[k]);
        fprintf(o, "\n");
    }
    fclose(o);
    return 0;
}
