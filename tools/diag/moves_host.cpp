// moves_host.cpp — the value of every root move (include/othello_moves.h,
// DESIGN.md §21) on the host: moves.hip's expand / tasks / finish scheme with a
// plain C++ statement of the rules, around the very cores the device runs
// (solve_core.hpp's machine for the exact rows, search_core.hpp's machine
// started by start_child() for the search's).
//
// Two uses, as search_host.cpp's:
//   * the scheme and the new start state can be run under
//     -fsanitize=address,undefined and compared against tests/moves_ref.py
//     before any GPU run;
//   * its per-position node counts are what the one-lane GPU calls must report.
//
// build:  g++ -O2 -std=c++17 -fopenmp -o tools/diag/moves_host tools/diag/moves_host.cpp
//         (-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all)
// run:    moves_host solve  IN OUT max_empties [node_limit=0] [threads=16]
//         moves_host search IN OUT WEIGHTS depth [node_limit=0] [threads=16]
//   IN : one position per line, "<black hex> <white hex> <turn>"
//   WEIGHTS: 36 integers in -128..127, [phase][feature]
//   OUT: one line per position, "<value> <best_move> <status> <nodes>" and the
//        row's 64 values
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../subproc_amd/csrc/search_core.hpp"
#include "../../subproc_amd/csrc/solve_core.hpp"
#include "host_io.hpp"
#include "host_rules.hpp"

typedef uint64_t u64;
typedef uint32_t u32;

constexpr u32 kDone = 1, kInvalid = 2, kSkipped = 0, kNoMove = 255, kPass = 64;
enum Kind { kMoves, kPassed, kOver, kBad, kSkip };

// a task: X to move against Y, the root mover's discs; sq the root move, 64 for the pass, 255 for an unused slot
struct Task {
    u64 X, Y;
    u32 sq;
    long value;
    u32 status, nodes;
};
struct Root {
    Kind kind;
    u32 count;
    size_t first;
};

// the expand step for one position: its tasks into t[0..], lowest square first
static Root expand(const Pos& p, int max_empties /* < 0: the search, no empties bound */, Task* t, size_t first) {
    Root r{kBad, 0, first};
    if (p.black & p.white) return r;
    if (max_empties >= 0 && 64 - HostRules::count(p.black | p.white) > max_empties) {
        r.kind = kSkip;
        return r;
    }
    const u64 P = p.mover(), O = p.other();
    u64 M = HostRules::moves(P, O);
    if (M == 0) {
        if (HostRules::moves(O, P) == 0) {
            r.kind = kOver;
            return r;
        }
        r.kind = kPassed;
        r.count = 1;
        t[0] = Task{O, P, kPass, 0, 0, 0};
        return r;
    }
    r.kind = kMoves;
    for (; M; M &= M - 1) {
        const u32 sq = HostRules::lowest(M);
        const u64 f = HostRules::flips(sq, P, O);
        t[r.count++] = Task{O & ~f, P | f | (1ull << sq), sq, 0, 0, 0};
    }
    return r;
}

// the finish step for one position
static void finish(const Pos& p, const Root& r, const Task* t, long scale, long not_a_move, long unknown, FILE* o) {
    long row[64];
    for (long& v : row) v = not_a_move;
    long best = LONG_MIN, value;
    u32 mv = kNoMove, st = kDone;
    unsigned long long nodes = r.count;
    bool unk = false;
    for (u32 j = 0; j < r.count; j++) {
        const long v = -t[j].value;
        nodes += t[j].nodes;
        if (t[j].status > st) st = t[j].status;
        if (t[j].status != kDone) {
            unk = true;
            if (t[j].sq < 64) row[t[j].sq] = unknown;
        } else {
            if (t[j].sq < 64) row[t[j].sq] = v;
            if (v > best) best = v, mv = t[j].sq;
        }
    }
    value = best;
    if (r.kind == kOver) {
        const long d = HostRules::count(p.black) - HostRules::count(p.white);
        value = scale * (p.turn == 2 ? -d : d);
    } else if (r.kind == kBad || r.kind == kSkip) {
        value = 0;
        st = r.kind == kBad ? kInvalid : kSkipped;
    } else if (unk) {
        value = 0;
        mv = kNoMove;
    }
    if (nodes > 0xFFFFFFFFull) nodes = 0xFFFFFFFFull;
    fprintf(o, "%ld %u %u %llu", value, mv, st, nodes);
    for (long v : row) fprintf(o, " %ld", v);
    fprintf(o, "\n");
}

static void solve_task(Task& t, u32 limit) {
    oths::Lane L;
    HostStack7<oths::kFrames> stk;
    oths::start(L, t.X, t.Y);
    while (L.depth >= 0) oths::advance<HostRules>(L, stk, limit);
    t.value = L.value, t.status = L.status, t.nodes = L.nodes;
}

// search_moves_kernel's claim: a depth-1 move task is a leaf scored on the spot
static void search_task(Task& t, int depth, const int* table, u32 limit) {
    const u64 cm = HostRules::moves(t.X, t.Y);
    if (t.sq != kPass && depth == 1) {
        const u64 om = HostRules::moves(t.Y, t.X);
        const int score = (cm | om) == 0 ? othm::kTerminal * (HostRules::count(t.Y) - HostRules::count(t.X))
                                         : othm::eval<HostRules>(table, t.Y, om, (u32)HostRules::count(t.X | t.Y));
        t.value = -(long)score, t.status = kDone, t.nodes = 0;
        return;
    }
    othm::Lane L;
    HostStack9<othm::kFrames> stk;
    othm::start_child(L, t.X, t.Y, cm, t.sq == kPass ? depth : depth - 1);
    while (L.depth >= 0) othm::advance<HostRules>(L, stk, table, limit);
    t.value = L.value, t.status = L.status, t.nodes = L.nodes;
}

int main(int argc, char** argv) {
    const bool solve = argc > 1 && !strcmp(argv[1], "solve"), search = argc > 1 && !strcmp(argv[1], "search");
    if ((!solve && !search) || argc < (solve ? 5 : 6)) {
        fprintf(stderr,
                "usage: %s solve IN OUT max_empties [node_limit] [threads]\n"
                "       %s search IN OUT WEIGHTS depth [node_limit] [threads]\n",
                argv[0], argv[0]);
        return 2;
    }
    const int opt = solve ? 5 : 6;
    const int level = atoi(argv[opt - 1]);  // max_empties or depth
    const u32 limit_arg = argc > opt ? (u32)strtoul(argv[opt], nullptr, 0) : 0u;
    const int threads = argc > opt + 1 ? atoi(argv[opt + 1]) : 16;
    const u32 limit = node_limit(limit_arg);
    if (threads < 1 || (solve && (level < 0 || level > oths::kMaxEmpties)) ||
        (search && (level < 1 || level > othm::kMaxDepth)))
        return 2;
    int table[othm::kEvalTable] = {0};
    if (search) read_weights(argv[4], table);
    std::vector<Pos> pos;
    read_positions(argv[2], 0, pos);
    const size_t n = pos.size();
    std::vector<Root> roots(n);
    std::vector<Task> tasks;
    size_t used;
    if (solve) {
        // a fixed max(max_empties, 1) slots per position; an unused slot is the empty board
        const size_t slots = level > 1 ? level : 1;
        tasks.assign(n * slots, Task{0, 0, kNoMove, 0, 0, 0});
        for (size_t i = 0; i < n; i++) roots[i] = expand(pos[i], level, tasks.data() + i * slots, i * slots);
        used = tasks.size();
    } else {
        // one packed list, sized for 64 tasks per position
        tasks.assign(n * 64, Task{0, 0, kNoMove, 0, 0, 0});
        used = 0;
        for (size_t i = 0; i < n; i++) {
            roots[i] = expand(pos[i], -1, tasks.data() + used, used);
            used += roots[i].count;
        }
    }
    const long total = (long)used;
#pragma omp parallel for schedule(dynamic, 16) num_threads(threads)
    for (long k = 0; k < total; k++) {
        Task& tk = tasks[k];
        if (solve) {
            // oths_solve's classification of a slot: the empty board has 64 empties and is skipped
            if (64 - HostRules::count(tk.X | tk.Y) > level)
                tk.status = kSkipped;
            else
                solve_task(tk, limit);
        } else {
            search_task(tk, level, table, limit);
        }
    }
    FILE* o = open_or_exit(argv[3], "w");
    for (size_t i = 0; i < n; i++) {
        if (solve)
            finish(pos[i], roots[i], tasks.data() + roots[i].first, 1, -128, -127, o);
        else
            finish(pos[i], roots[i], tasks.data() + roots[i].first, othm::kTerminal, (long)INT32_MIN,
                   (long)INT32_MIN + 1, o);
    }
    fclose(o);
    return 0;
}
