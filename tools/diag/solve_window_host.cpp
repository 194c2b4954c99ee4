// solve_window_host.cpp — the exact solvers' ROOT WINDOW on the host (DESIGN.md
// §20): solve_core.hpp's one-lane machine started with a window, and
// solve_tree_core.hpp's split tree whose root hands its window down, with a
// plain C++ statement of the rules.  The very cores the device runs.
//
// mode a  ONE THREAD PER POSITION (OpenMP over the input's lines, each line's
//         work by one thread), plain loads and stores.  Per position and window:
//         the one-lane machine, its node count under the full window, and the
//         split cores in four task orders (forward, reverse, a seeded shuffle,
//         all with shared bounds, and forward with the windows fixed before any
//         task runs) under both move orders.  All nine must give the same
//         value, move and status.
// mode b  `threads` std::thread workers take a position's tasks off one counter
//         and share the tree's state words and ONE transposition table through
//         __atomic accesses that carry the device's orderings (as
//         solve_hash_host.cpp's mode b).  Two passes over the input on the one
//         table nothing clears: phase 0 = every position under the FULL window,
//         then under its own; phase 1 = the other way round.
//
// build:  g++ -O2 -std=c++17 -pthread -fopenmp -o tools/diag/solve_window_host tools/diag/solve_window_host.cpp
//         (-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all for mode a,
//          -O1 -g -fsanitize=thread for mode b)
// run:    solve_window_host a IN OUT max_empties task_empties nodes_per_position [threads=1] [seed=7] [node_limit=0]
//         solve_window_host b IN OUT max_empties task_empties nodes_per_position order hash_bits hash_min_empties
//                           phase [threads=8] [node_limit=0]
//   IN : one position per line, "<black hex> <white hex> <turn> <alpha> <beta>"
//   OUT: mode a: per line "<value> <move> <status> <nodes> <full-window nodes>" of the one-lane machine, then
//                eight times "<value> <move> <status>": move order 0 then 1, each in the four task orders
//        mode b: per line "<value> <move> <status>" under the line's window, then under the full window
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "../../subproc_amd/csrc/solve_hash_core.hpp"
#include "../../subproc_amd/csrc/solve_tree_core.hpp"
#include "host_io.hpp"
#include "host_rules.hpp"

using othe::Node;
using othe::u32;
using othe::u64;

using HostStack = HostStack7<oths::kFrames>;

// solve_hash_host.cpp's mode b policies: the orderings solve_hash_core.hpp asks for, each on its access
struct ThreadHashAtomics {
    static u64 load(u64* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
    static u64 seq_load(u64* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
    static u64 data_load(u64* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
    static void read_fence() {}
    static bool claim(u64* p, u64 expected, u64 desired) {
        return __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED);
    }
    static void data_store(u64* p, u64 v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }
    static void publish(u64* p, u64 v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }
};
struct ThreadTreeAtomics {
    static u64 load(u64* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
    static bool cas(u64* p, u64& expected, u64 desired) {
        return __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE);
    }
    static void store(u64* p, u64 v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }
};

// the line's window: its two extra columns
static int alpha_of(const Pos& p) { return (int)p.extra[0]; }
static int beta_of(const Pos& p) { return (int)p.extra[1]; }
struct Out {
    int value;
    u32 best, status;
    u64 nodes;
};

// what solve.hip's and solve_tree.hip's kernels decide before any search
static u32 classify(const Pos& p, int max_empties, int ra, int rb) {
    const u32 cls = oths::classify(p.black, p.white, 64 - HostRules::count(p.black | p.white), max_empties);
    return cls == oths::kSolved && !oths::window_ok(ra, rb) ? oths::kBadWindow : cls;
}

// solve.hip's windowed kernel for one position
static Out solve_lane(const Pos& p, int max_empties, u32 limit, int ra, int rb) {
    const u32 cls = classify(p, max_empties, ra, rb);
    if (cls != oths::kSolved) return Out{0, oths::kNoMove, cls, 0};
    oths::Lane L;
    HostStack stk;
    oths::start(L, p.mover(), p.other(), ra, rb);
    while (L.depth >= 0) oths::advance<HostRules>(L, stk, limit);
    if (L.status == oths::kSolved) L.value = oths::clamp_to_window(L.value, ra, rb);
    return Out{L.value, L.best_mv, L.status, L.nodes};
}

// solve_tree.hip's expansion for one position under the root window (ra, rb).
// False: `out` is the answer already.
static bool expand(const Pos& p, int max_empties, int task_empties, u32 npp, int ra, int rb, std::vector<Node>& slab,
                   std::vector<u32>& tasks, Out& out) {
    const u32 cls = classify(p, max_empties, ra, rb);
    if (cls != oths::kSolved) {
        out = Out{0, oths::kNoMove, cls, 0};
        return false;
    }
    if (slab.size() != npp) slab.assign(npp, Node{});  // (every node used below is made whole first)
    tasks.clear();
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
    bool deep = false;
    for (u32 i = 0; i < end; i++)
        if (othe::is_task(slab[i])) {
            tasks.push_back(i);
            deep |= slab[i].emp > oths::kMaxEmpties;
        }
    out = Out{0, oths::kNoMove, oths::kSolved, (u64)end - 1};
    if (deep) {
        out.status = othe::kNoRoom;
        return false;
    }
    if (tasks.empty()) {
        othe::root_result_window<HostAtomics>(slab.data(), out.value, out.best, out.status, ra, rb);
        return false;
    }
    return true;
}

// one task, as a lane of the task kernel runs it (tab == nullptr: the unhashed
// machines).  True in `root` when this task completed the root.
template <class TA, class HA>
static void run_task(Node* slab, u32 t, bool shared, int ra, int rb, const othh::Table* tab, int ordered, u32 limit,
                     Out& out, bool& root) {
    int alpha, beta, v;
    u64 lim = 0;
    othe::window_rooted<TA>(slab, t, shared, alpha, beta, ra, rb);
    if (alpha < -othe::kInf || beta > othe::kInf) {  // a window the int8 halves cannot hold: a defect
        fprintf(stderr, "task window (%d, %d)\n", alpha, beta);
        abort();
    }
    if (alpha >= beta) {
        v = beta;
    } else {
        oths::Lane L;
        HostStack stk;
        othe::start_task(L, slab[t], alpha, beta);
        othm::Order Q;
        othm::order_reset(Q);
        if (tab && ordered)
            while (L.depth >= 0) othh::advance_ordered_hashed<HostRules, HA>(L, Q, stk, *tab, limit);
        else if (tab)
            while (L.depth >= 0) othh::advance_hashed<HostRules, HA>(L, stk, *tab, limit);
        else if (ordered)
            while (L.depth >= 0) oths::advance_ordered<HostRules>(L, Q, stk, limit);
        else
            while (L.depth >= 0) oths::advance<HostRules>(L, stk, limit);
        v = L.value;
        lim = L.status == oths::kLimit ? othe::kLimitBit : 0;
    }
    root = othe::fold_up<TA>(slab, t, v, lim);
    if (root) othe::root_result_window<TA>(slab, out.value, out.best, out.status, ra, rb);
}

enum Order { kForward, kReverse, kShuffle, kSnapshot };

// mode a: the tasks one after the other
static Out solve_serial(const std::vector<Node>& tree, std::vector<u32> tasks, Out out, Order order, u32 seed, int ra,
                        int rb, int ordered, u32 limit) {
    std::vector<Node> slab(tree.begin(), tree.begin() + (size_t)out.nodes + 1);  // the expansion's nodes
    if (order == kReverse) std::reverse(tasks.begin(), tasks.end());
    if (order == kShuffle) {
        std::mt19937 rng(seed);
        for (size_t i = tasks.size(); i > 1; i--) std::swap(tasks[i - 1], tasks[rng() % i]);
    }
    bool emitted = false;
    for (u32 t : tasks) {
        if (emitted) return Out{0, 0, 99, 0};  // the root completed before the last task: a defect
        run_task<HostAtomics, ThreadHashAtomics>(slab.data(), t, order != kSnapshot, ra, rb, nullptr, ordered, limit, out,
                                                 emitted);
    }
    if (!emitted) return Out{0, 0, 98, 0};  // the root never completed: a defect
    return out;
}

// mode b: `threads` workers take the tasks off one counter
static Out solve_threads(std::vector<Node>& slab, const std::vector<u32>& tasks, Out out, int threads, int ra, int rb,
                         const othh::Table* tab, int ordered, u32 limit) {
    std::atomic<size_t> next{0};
    std::atomic<int> emitted{0};
    Out answer = out;
    std::vector<std::thread> pool;
    for (int k = 0; k < threads; k++)
        pool.emplace_back([&] {
            for (;;) {
                const size_t i = next.fetch_add(1);
                if (i >= tasks.size()) return;
                Out mine = out;
                bool root = false;
                run_task<ThreadTreeAtomics, ThreadHashAtomics>(slab.data(), tasks[i], true, ra, rb, tab, ordered, limit,
                                                               mine, root);
                if (root) {
                    answer = mine;  // (one thread only: the joins below publish it)
                    emitted++;
                }
            }
        });
    for (auto& th : pool) th.join();
    if (emitted.load() != 1) return Out{0, 0, 98, 0};  // the root completed never, or twice: a defect
    return answer;
}

int main(int argc, char** argv) {
    if (argc < 7) {
        fprintf(stderr,
                "usage: %s a IN OUT max_empties task_empties nodes_per_position [threads] [seed] [node_limit]\n"
                "       %s b IN OUT max_empties task_empties nodes_per_position order hash_bits hash_min_empties phase "
                "[threads] [node_limit]\n",
                argv[0], argv[0]);
        return 2;
    }
    const char mode = argv[1][0];
    const int max_empties = atoi(argv[4]), task_empties = atoi(argv[5]);
    const long npp = atol(argv[6]);
    if ((mode != 'a' && mode != 'b') || (mode == 'b' && argc < 11)) return 2;
    if (max_empties < 0 || max_empties > othe::kMaxEmpties || task_empties < 1 || task_empties > oths::kMaxEmpties ||
        npp < othe::kMinNodes || npp > (1 << 24))
        return 2;
    std::vector<Pos> pos;
    read_positions(argv[2], 2, pos);
    FILE* o = open_or_exit(argv[3], "w");
    std::vector<Node> tree;
    std::vector<u32> tasks;
    if (mode == 'a') {
        const int threads = argc > 7 ? atoi(argv[7]) : 1;
        const u32 seed = argc > 8 ? (u32)strtoul(argv[8], nullptr, 0) : 7u;
        const u32 limit_arg = argc > 9 ? (u32)strtoul(argv[9], nullptr, 0) : 0u;
        const u32 limit = node_limit(limit_arg);
        if (threads < 1 || threads > 64) return 2;
        const long n = (long)pos.size();
        std::vector<Out> res((size_t)n * 10);  // the lane, the lane under the full window, the eight split runs
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads) firstprivate(tree, tasks)
        for (long i = 0; i < n; i++) {
            const Pos& p = pos[i];
            // (the one-lane machine takes 12 empties at most: above, its columns are a skipped position's)
            const int lane_empties = std::min(max_empties, oths::kMaxEmpties);
            res[i * 10] = solve_lane(p, lane_empties, limit, alpha_of(p), beta_of(p));
            res[i * 10 + 1] = solve_lane(p, lane_empties, limit, -oths::kInf, oths::kInf);
            Out first;
            const bool run = expand(p, max_empties, task_empties, (u32)npp, alpha_of(p), beta_of(p), tree, tasks, first);
            for (int ordered = 0; ordered < 2; ordered++)
                for (int order = 0; order < 4; order++)
                    res[i * 10 + 2 + ordered * 4 + order] =
                        run ? solve_serial(tree, tasks, first, (Order)order, seed, alpha_of(p), beta_of(p), ordered, limit) : first;
        }
        for (long i = 0; i < n; i++) {
            const Out &one = res[i * 10], &full = res[i * 10 + 1];
            fprintf(o, "%d %u %u %llu %llu", one.value, one.best, one.status, (unsigned long long)one.nodes,
                    (unsigned long long)full.nodes);
            for (int k = 2; k < 10; k++) fprintf(o, " %d %u %u", res[i * 10 + k].value, res[i * 10 + k].best, res[i * 10 + k].status);
            fprintf(o, "\n");
        }
        fclose(o);
        return 0;
    }
    const int ordered = atoi(argv[7]), bits = atoi(argv[8]), gate = atoi(argv[9]), phase = atoi(argv[10]);
    const int threads = argc > 11 ? atoi(argv[11]) : 8;
    const u32 limit_arg = argc > 12 ? (u32)strtoul(argv[12], nullptr, 0) : 0u;
    const u32 limit = node_limit(limit_arg);
    if (ordered < 0 || ordered > 1 || phase < 0 || phase > 1 || threads < 1 || threads > 64) return 2;
    if (bits < othh::kMinBits || bits > 24 || gate < othh::kMinGate || gate > othh::kMaxGate) return 2;
    std::vector<othh::Entry> entries((size_t)1 << bits);  // all zero: empty; never cleared below
    othh::Table tab;
    tab.e = entries.data();
    tab.shift = 64 - bits;
    tab.min_empties = gate;
    std::vector<Out> res(pos.size() * 2);  // [position][0: its window, 1: the full one]
    for (int pass = 0; pass < 2; pass++) {
        const bool full = (pass == 0) == (phase == 0);
        for (size_t i = 0; i < pos.size(); i++) {
            const int ra = full ? -othe::kInf : alpha_of(pos[i]), rb = full ? othe::kInf : beta_of(pos[i]);
            Out first;
            const bool run = expand(pos[i], max_empties, task_empties, (u32)npp, ra, rb, tree, tasks, first);
            res[i * 2 + (full ? 1 : 0)] = run ? solve_threads(tree, tasks, first, threads, ra, rb, &tab, ordered, limit) : first;
        }
    }
    for (size_t i = 0; i < pos.size(); i++)
        fprintf(o, "%d %u %u %d %u %u\n", res[i * 2].value, res[i * 2].best, res[i * 2].status, res[i * 2 + 1].value,
                res[i * 2 + 1].best, res[i * 2 + 1].status);
    fclose(o);
    return 0;
}
