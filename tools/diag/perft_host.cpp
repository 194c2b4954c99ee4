// perft_host.cpp — perft (include/othello_perft.h) on the host:
// the very machine the device runs (perft_core.hpp) with a plain C++ statement
// of the rules, inside a plain restatement of perft.hip's scheme: one task per
// valid position, `split` levels of expansion between two lists of `max_tasks`
// tasks (a level that does not fit is void and the level before it stays in
// force), the machine on every task of the last level, the finish.
//
// Two uses, as moves_host.cpp's:
//   * the machine and the scheme can be run under -fsanitize=address,undefined
//     and compared against tests/perft_ref.py before any GPU run;
//   * with threads it is the host baseline of tools/perft_bench.py.
//
// build:  g++ -O2 -std=c++17 -fopenmp -o tools/diag/perft_host tools/diag/perft_host.cpp
//         (-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all)
// run:    perft_host IN OUT depth split max_tasks [divide=1] [node_limit=0] [threads=16]
//   IN : one position per line, "<black hex> <white hex> <turn> [<depth>]"
//        (budget_host.cpp's format); depth < 0 on the command line takes each
//        position's own from its line
//   divide=1: the rows are computed, which asks for at least one level and for
//        lists of 64 tasks per position (othc_perft refuses smaller ones; here
//        they are raised, as ops.perft raises them)
//   OUT: one line per position, "<leaves> <status> <nodes>" and the row's 64
//        counts; then one line "levels <made> void <first void level or 0> tasks <of the level counted>"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../subproc_amd/csrc/perft_core.hpp"
#include "host_io.hpp"
#include "host_rules.hpp"

typedef uint64_t u64;
typedef uint32_t u32;

// perft_core.hpp's frames
struct HostStack6 {
    u64 P[othc::kFrames], O[othc::kFrames], M[othc::kFrames];
    void store(int d, u64 p, u64 o, u64 m) { P[d] = p, O[d] = o, M[d] = m; }
    void load(int d, u64& p, u64& o, u64& m) const { p = P[d], o = O[d], m = M[d]; }
};

struct Task {
    u64 P, O, word;
};

// what replaces task t at the next level, appended to `out`
static void expand(const Task& t, std::vector<Task>& out) {
    if (othc::task_final(t.word)) {
        out.push_back(t);
        return;
    }
    const u64 index = othc::task_index(t.word);
    const u32 sq0 = othc::task_sq(t.word), rem = othc::task_rem(t.word);
    u64 M = HostRules::moves(t.P, t.O);
    if (M == 0) {
        if (HostRules::moves(t.O, t.P))  // a pass is a ply
            out.push_back(Task{t.O, t.P, othc::task_word(index, sq0 == othc::kSqNone ? othc::kSqPass : sq0, rem - 1, false)});
        else
            out.push_back(Task{t.P, t.O, othc::task_word(index, sq0, rem, true)});
        return;
    }
    for (; M; M &= M - 1) {
        const u32 sq = HostRules::lowest(M);
        const u64 f = HostRules::flips(sq, t.P, t.O);
        out.push_back(Task{t.O & ~f, t.P | f | (1ull << sq), othc::task_word(index, sq0 == othc::kSqNone ? sq : sq0, rem - 1, false)});
    }
}

int main(int argc, char** argv) {
    if (argc < 6) usage(argv[0], "IN OUT depth split max_tasks [divide=1] [node_limit=0] [threads=16]");
    const int depth = atoi(argv[3]), split = atoi(argv[4]);
    const long max_tasks = atol(argv[5]);
    const bool divide = argc > 6 ? atoi(argv[6]) != 0 : true;
    const u32 limit_arg = argc > 7 ? (u32)strtoul(argv[7], nullptr, 0) : 0u;
    const int threads = argc > 8 ? atoi(argv[8]) : 16;
    const u32 limit = node_limit(limit_arg);
    if (depth > othc::kMaxDepth || split < 0 || split > 8 || max_tasks < 0 || max_tasks > (1l << 24) || threads < 1)
        return 2;
    FILE* in = open_or_exit(argv[1], "r");
    std::vector<Pos> pos;
    std::vector<int> depths;  // each position's own, or the command line's
    char line[256];
    while (fgets(line, sizeof line, in)) {
        Pos p;
        const int got = parse_position(line, p);
        if (got < 3) continue;
        if (depth < 0 && got < 4) return 2;
        pos.push_back(p);
        depths.push_back(depth < 0 ? (int)p.extra[0] : depth);
    }
    fclose(in);
    const size_t n = pos.size();
    if (n > (1u << 24)) return 2;
    const size_t cap = std::max<size_t>(std::max<size_t>((size_t)max_tasks, n) , divide ? 64 * n : 1);
    const int levels = std::max(split, divide ? 1 : 0);

    // level 0: one task per valid position
    std::vector<Task> list, next;
    for (size_t i = 0; i < n; i++) {
        const Pos& p = pos[i];
        if ((p.black & p.white) || depths[i] < 0 || depths[i] > othc::kMaxDepth) continue;
        list.push_back(Task{p.mover(), p.other(), othc::task_word(i, othc::kSqNone, (u32)depths[i], false)});
    }
    int made = 0, first_void = 0;
    for (int k = 1; k <= levels; k++) {
        next.clear();
        bool fits = true;
        for (const Task& t : list) {
            expand(t, next);
            if (next.size() > cap) {  // the level is void: the list in force stays, later levels are not made
                fits = false;
                break;
            }
        }
        if (!fits) {
            first_void = k;
            break;
        }
        list.swap(next);
        made = k;
    }

    std::vector<u64> leaves(n, 0), nodes(n, 0), row(n * 64, 0);
    std::vector<unsigned char> hit(n, 0);
    const long total = (long)list.size();
#pragma omp parallel for schedule(dynamic, 16) num_threads(threads)
    for (long k = 0; k < total; k++) {
        const Task& t = list[k];
        const u64 i = othc::task_index(t.word);
        const u32 sq = othc::task_sq(t.word);
        u64 count = 1;
        u32 visited = 0, status = othc::kCounted;
        if (!othc::task_final(t.word)) {
            othc::Lane L;
            HostStack6 stk;
            othc::start(L, t.P, t.O, (int)othc::task_rem(t.word));
            while (L.depth >= 0) othc::advance<HostRules>(L, stk, limit);
            count = L.count, visited = L.nodes, status = L.status;
        }
#pragma omp atomic
        nodes[i] += visited;
        if (status == othc::kLimit) {
#pragma omp atomic write
            hit[i] = 1;
            continue;
        }
#pragma omp atomic
        leaves[i] += count;
        if (divide && sq < 64) {
#pragma omp atomic
            row[i * 64 + sq] += count;
        }
    }

    FILE* o = open_or_exit(argv[2], "w");
    for (size_t i = 0; i < n; i++) {
        const Pos& p = pos[i];
        const u32 st = (p.black & p.white)                              ? othc::kInvalid
                       : (depths[i] < 0 || depths[i] > othc::kMaxDepth) ? othc::kBadDepth
                       : hit[i]                                         ? othc::kLimit
                                                                        : othc::kCounted;
        fprintf(o, "%llu %u %llu", (unsigned long long)(hit[i] ? 0 : leaves[i]), st, (unsigned long long)nodes[i]);
        for (int s = 0; s < 64; s++) fprintf(o, " %llu", (unsigned long long)(hit[i] ? 0 : row[i * 64 + s]));
        fprintf(o, "\n");
    }
    fprintf(o, "levels %d void %d tasks %ld\n", made, first_void, total);
    fclose(o);
    return 0;
}
