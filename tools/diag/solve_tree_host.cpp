// solve_tree_host.cpp — the split solver's tree (subproc_amd/csrc/solve_tree_core.hpp)
// and the one-lane state machines below it (solve_core.hpp, solve_order_core.hpp)
// on the host, with a plain C++ statement of the rules and plain loads and
// stores for the atomics.
//
// The expansion, the back-up and the windows are solve_tree_core.hpp's, so the
// tie rule and the empty-window rule of DESIGN.md §15 / §17 can be run under
// -fsanitize=address,undefined and compared against tests/solve_ref.py and the
// deep fixture before any GPU run.  Each position's tasks are run in four
// orders: forward, reverse, a seeded shuffle (all with shared bounds), and
// forward with the windows fixed before any task runs ("nothing shared").  All
// four must give the same value, move and status.  The forward order is also
// the one-lane node count the GPU's split is priced against.
//
// build:  g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all
//             -o tools/diag/solve_tree_host_asan tools/diag/solve_tree_host.cpp
//         (-O2 -fopenmp for the timed 16-thread runs of tools/solve_tree_bench.py)
// run:    solve_tree_host IN OUT max_empties task_empties [nodes_per_position=65536] [node_limit=0] [seed=1]
//                         [order=0] [threads=1] [task_orders=4]
//   IN : one position per line, "<black hex> <white hex> <turn>"
//   OUT: one line per position, task_orders times "<value> <best_move> <status> <nodes>"
//   stderr: one JSON line with the wall time
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../subproc_amd/csrc/solve_order_core.hpp"
#include "../../subproc_amd/csrc/solve_tree_core.hpp"
#include "host_io.hpp"
#include "host_rules.hpp"

using othe::Node;
using othe::u32;
using othe::u64;

using HostStack = HostStack7<oths::kFrames>;

struct Out {
    int value;
    u32 best, status;
    u64 nodes;
};

enum Order { kForward, kReverse, kShuffle, kSnapshot };

// solve_tree.hip's expansion and task kernels for one position, one task at a time
static Out solve_one(const Pos& p, int max_empties, int task_empties, u32 npp, u32 limit, Order order, u32 seed,
                     int ordered) {
    const u32 cls = oths::classify(p.black, p.white, 64 - HostRules::count(p.black | p.white), max_empties);
    if (cls != oths::kSolved) return Out{0, oths::kNoMove, cls, 0};
    std::vector<Node> slab(npp);
    othe::make_node<HostRules>(slab[0], p.mover(), p.other(), -1, oths::kNoMove);
    u32 lvl[othe::kMaxRounds + 2] = {0, 1};
    u32 begin = 0, end = 1;
    int rounds = 0;
    while (rounds < othe::kMaxRounds) {
        u64 total = 0;
        for (u32 i = begin; i < end; i++) total += othe::child_count<HostRules>(slab[i], task_empties);
        if (total == 0 || end + total > npp) break;
        u32 at = end;
        for (u32 i = begin; i < end; i++) {
            const u32 c = othe::child_count<HostRules>(slab[i], task_empties);
            if (c) othe::expand<HostRules>(slab.data(), i, at, c);
            at += c;
        }
        begin = end;
        end += (u32)total;
        lvl[++rounds + 1] = end;
    }
    for (int r = rounds; r >= 1; r--)
        for (u32 i = lvl[r]; i < lvl[r + 1]; i++) {
            const u64 w = slab[i].state;
            if ((slab[i].flags & othe::kFinal) || (slab[i].nchild && othe::count_of(w) == 0))
                othe::fold<HostAtomics>(slab.data(), (u32)slab[i].parent, othe::best_of(w), 0);
        }
    for (u32 i = 0; i < end; i++) slab[i].snap = othe::best_of(slab[i].state);
    std::vector<u32> tasks;
    bool deep = false;
    for (u32 i = 0; i < end; i++)
        if (othe::is_task(slab[i])) {
            tasks.push_back(i);
            deep |= slab[i].emp > oths::kMaxEmpties;
        }
    u64 nodes = end - 1;
    if (deep) return Out{0, oths::kNoMove, othe::kNoRoom, nodes};
    Out out{0, oths::kNoMove, oths::kSolved, nodes};
    if (tasks.empty()) {
        othe::root_result<HostAtomics>(slab.data(), out.value, out.best, out.status);
        return out;
    }
    if (order == kReverse) std::reverse(tasks.begin(), tasks.end());
    if (order == kShuffle) {
        std::mt19937 rng(seed);
        for (size_t i = tasks.size(); i > 1; i--) std::swap(tasks[i - 1], tasks[rng() % i]);
    }
    bool emitted = false;
    for (u32 t : tasks) {
        int alpha, beta, v;
        u64 lim = 0;
        othe::window<HostAtomics>(slab.data(), t, order != kSnapshot, alpha, beta);
        if (alpha < -othe::kInf || beta > othe::kInf) return Out{0, 0, 97, 0};  // a window the int8 halves cannot hold: a defect
        if (alpha >= beta) {
            v = beta;
        } else {
            oths::Lane L;
            HostStack stk;
            othe::start_task(L, slab[t], alpha, beta);
            othm::Order Q;
            othm::order_reset(Q);
            if (ordered)
                while (L.depth >= 0) oths::advance_ordered<HostRules>(L, Q, stk, limit);
            else
                while (L.depth >= 0) oths::advance<HostRules>(L, stk, limit);
            v = L.value;
            lim = L.status == oths::kLimit ? othe::kLimitBit : 0;
            nodes += L.nodes;
        }
        if (emitted) return Out{0, 0, 99, 0};  // the root completed before the last task: a defect
        if (othe::fold_up<HostAtomics>(slab.data(), t, v, lim)) {
            othe::root_result<HostAtomics>(slab.data(), out.value, out.best, out.status);
            emitted = true;
        }
    }
    if (!emitted) return Out{0, 0, 98, 0};  // the root never completed: a defect
    out.nodes = nodes;
    return out;
}

int main(int argc, char** argv) {
    if (argc < 5)
        usage(argv[0],
              "IN OUT max_empties task_empties [nodes_per_position] [node_limit] [seed] [order] [threads] [task_orders]");
    const int max_empties = atoi(argv[3]), task_empties = atoi(argv[4]);
    const long npp = argc > 5 ? atol(argv[5]) : 65536;
    const u32 limit_arg = argc > 6 ? (u32)strtoul(argv[6], nullptr, 0) : 0u;
    const u32 seed = argc > 7 ? (u32)strtoul(argv[7], nullptr, 0) : 1u;
    const int ordered = argc > 8 ? atoi(argv[8]) : 0;
    const int threads = argc > 9 ? atoi(argv[9]) : 1;
    const int norders = argc > 10 ? atoi(argv[10]) : 4;
    if (ordered < 0 || ordered > 1 || threads < 1 || norders < 1 || norders > 4) return 2;
    if (max_empties < 0 || max_empties > othe::kMaxEmpties || task_empties < 1 || task_empties > oths::kMaxEmpties ||
        npp < othe::kMinNodes || npp > (1 << 24))
        return 2;
    const u32 limit = node_limit(limit_arg);
    std::vector<Pos> pos;
    read_positions(argv[1], 0, pos);
    const long n = (long)pos.size();
    std::vector<Out> out((size_t)n * norders);
    const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long i = 0; i < n; i++)
        for (int order = 0; order < norders; order++)
            out[(size_t)i * norders + order] =
                solve_one(pos[i], max_empties, task_empties, (u32)npp, limit, (Order)order, seed, ordered);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    FILE* o = open_or_exit(argv[2], "w");
    unsigned long long nodes = 0;
    for (long i = 0; i < n; i++)
        for (int order = 0; order < norders; order++) {
            const Out& r = out[(size_t)i * norders + order];
            fprintf(o, "%d %u %u %llu%s", r.value, r.best, r.status, (unsigned long long)r.nodes,
                    order == norders - 1 ? "\n" : " ");
            if (order == 0) nodes += r.nodes;
        }
    fclose(o);
    fprintf(stderr, "{\"positions\": %ld, \"threads\": %d, \"seconds\": %.6f, \"forward_nodes\": %llu}\n", n, threads, sec,
            nodes);
    return 0;
}
