// solve_hash_host.cpp — the split solver's transposition table
// (subproc_amd/csrc/solve_hash_core.hpp) on the host: the very probe, store and
// hashed state machines the device runs, below solve_tree_core.hpp's tree, with
// a plain C++ statement of the rules.  DESIGN.md §19.
//
// mode a  ONE THREAD, plain loads and stores.  Each position's tasks are run in
//         up to three orders (forward, reverse, a seeded shuffle) on ONE table
//         that all positions and all orders share and nothing ever clears, then
//         (plain = 1) once more forward WITHOUT the table.  Every run must give
//         the same value, move and status; the forward runs' node counts are the
//         subset property's two sides (hashed <= unhashed, root by root).
// mode b  `threads` std::thread workers take a position's tasks off one counter
//         and share the tree's state words and the table through __atomic
//         accesses that carry the device's orderings ON THE ACCESSES (the
//         device spells them with fences, which ThreadSanitizer does not model;
//         solve_hash_core.hpp states what either spelling must give).
//
// build:  g++ -O2 -std=c++17 -pthread -o tools/diag/solve_hash_host tools/diag/solve_hash_host.cpp
//         (-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all for mode a,
//          -O1 -g -fsanitize=thread for mode b: tools/diag/solve_hash_host_check.py runs both)
// run:    solve_hash_host MODE IN OUT max_empties task_empties nodes_per_position order hash_bits hash_min_empties
//                         [task_orders=3] [plain=1] [threads=8] [seed=7] [node_limit=0]
//   IN : one position per line, "<black hex> <white hex> <turn>"
//   OUT: mode a: per position, task_orders times "<value> <best_move> <status> <nodes>", then the same four of
//                the run without the table when plain = 1
//        mode b: per position "<value> <best_move> <status> <nodes>"
//   stderr: one JSON line: wall time, the forward runs' nodes with and without the table
#include <algorithm>
#include <atomic>
#include <chrono>
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

// mode a: one thread touches the table at a time
struct PlainHashAtomics {
    static u64 load(u64* p) { return *p; }
    static u64 seq_load(u64* p) { return *p; }
    static u64 data_load(u64* p) { return *p; }
    static void read_fence() {}
    static bool claim(u64* p, u64 expected, u64 desired) {
        if (*p != expected) return false;
        *p = desired;
        return true;
    }
    static void data_store(u64* p, u64 v) { *p = v; }
    static void publish(u64* p, u64 v) { *p = v; }
};

// mode b: the orderings solve_hash_core.hpp asks for, each on its access
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

// mode b: the tree's state words
struct ThreadTreeAtomics {
    static u64 load(u64* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
    static bool cas(u64* p, u64& expected, u64 desired) {
        return __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE);
    }
    static void store(u64* p, u64 v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }
};

struct Out {
    int value;
    u32 best, status;
    u64 nodes;
};

// solve_tree.hip's expansion for one position.  False: `out` is the answer
// already (skipped, invalid, no room, or the game ends inside the expanded plies).
static bool expand(const Pos& p, int max_empties, int task_empties, u32 npp, std::vector<Node>& slab,
                   std::vector<u32>& tasks, Out& out) {
    const u32 cls = oths::classify(p.black, p.white, 64 - HostRules::count(p.black | p.white), max_empties);
    if (cls != oths::kSolved) {
        out = Out{0, oths::kNoMove, cls, 0};
        return false;
    }
    slab.assign(npp, Node{});
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
        othe::root_result<HostAtomics>(slab.data(), out.value, out.best, out.status);
        return false;
    }
    return true;
}

// one task, as a lane of the task kernel runs it.  tab == nullptr: the
// unhashed machines.  Returns the task's nodes; true in `root` when this task
// completed the root (then `out` has the answer).
template <class TA, class HA>
static u64 run_task(Node* slab, u32 t, const othh::Table* tab, int ordered, u32 limit, Out& out, bool& root) {
    int alpha, beta, v;
    u64 lim = 0, nodes = 0;
    othe::window<TA>(slab, t, true, alpha, beta);
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
        nodes = L.nodes;
    }
    root = othe::fold_up<TA>(slab, t, v, lim);
    if (root) othe::root_result<TA>(slab, out.value, out.best, out.status);
    return nodes;
}

// mode a: the tasks one after the other, in the given order
static Out solve_serial(const std::vector<Node>& tree, std::vector<u32> tasks, Out out, int order, u32 seed,
                        const othh::Table* tab, int ordered, u32 limit) {
    std::vector<Node> slab = tree;
    if (order == 1) std::reverse(tasks.begin(), tasks.end());
    if (order == 2) {
        std::mt19937 rng(seed);
        for (size_t i = tasks.size(); i > 1; i--) std::swap(tasks[i - 1], tasks[rng() % i]);
    }
    bool emitted = false;
    for (u32 t : tasks) {
        if (emitted) return Out{0, 0, 99, 0};  // the root completed before the last task: a defect
        out.nodes += run_task<HostAtomics, PlainHashAtomics>(slab.data(), t, tab, ordered, limit, out, emitted);
    }
    if (!emitted) return Out{0, 0, 98, 0};  // the root never completed: a defect
    return out;
}

// mode b: `threads` workers take the tasks off one counter
static Out solve_threads(std::vector<Node>& slab, const std::vector<u32>& tasks, Out out, int threads,
                         const othh::Table* tab, int ordered, u32 limit) {
    std::atomic<size_t> next{0};
    std::atomic<u64> nodes{0};
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
                nodes += run_task<ThreadTreeAtomics, ThreadHashAtomics>(slab.data(), tasks[i], tab, ordered, limit, mine,
                                                                        root);
                if (root) {
                    answer = mine;  // (one thread only: the joins below publish it)
                    emitted++;
                }
            }
        });
    for (auto& th : pool) th.join();
    if (emitted.load() != 1) return Out{0, 0, 98, 0};  // the root completed never, or twice: a defect
    answer.nodes = out.nodes + nodes.load();
    return answer;
}

int main(int argc, char** argv) {
    if (argc < 10)
        usage(argv[0],
              "a|b IN OUT max_empties task_empties nodes_per_position order hash_bits hash_min_empties "
              "[task_orders] [plain] [threads] [seed] [node_limit]");
    const char mode = argv[1][0];
    const int max_empties = atoi(argv[4]), task_empties = atoi(argv[5]);
    const long npp = atol(argv[6]);
    const int ordered = atoi(argv[7]), bits = atoi(argv[8]), gate = atoi(argv[9]);
    const int norders = argc > 10 ? atoi(argv[10]) : 3;
    const int plain = argc > 11 ? atoi(argv[11]) : 1;
    const int threads = argc > 12 ? atoi(argv[12]) : 8;
    const u32 seed = argc > 13 ? (u32)strtoul(argv[13], nullptr, 0) : 7u;
    const u32 limit_arg = argc > 14 ? (u32)strtoul(argv[14], nullptr, 0) : 0u;
    if ((mode != 'a' && mode != 'b') || ordered < 0 || ordered > 1 || threads < 1 || threads > 64 || norders < 1 ||
        norders > 3 || plain < 0 || plain > 1)
        return 2;
    if (max_empties < 0 || max_empties > othe::kMaxEmpties || task_empties < 1 || task_empties > oths::kMaxEmpties ||
        npp < othe::kMinNodes || npp > (1 << 24))
        return 2;
    if (bits < othh::kMinBits || bits > 24 || gate < othh::kMinGate || gate > othh::kMaxGate) return 2;
    const u32 limit = node_limit(limit_arg);
    std::vector<Pos> pos;
    read_positions(argv[2], 0, pos);
    std::vector<othh::Entry> entries((size_t)1 << bits);  // all zero: empty; never cleared below
    othh::Table tab;
    tab.e = entries.data();
    tab.shift = 64 - bits;
    tab.min_empties = gate;
    FILE* o = open_or_exit(argv[3], "w");
    unsigned long long hashed = 0, unhashed = 0;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<Node> tree;
    std::vector<u32> tasks;
    for (const Pos& p : pos) {
        Out first;
        const bool run = expand(p, max_empties, task_empties, (u32)npp, tree, tasks, first);
        if (mode == 'b') {
            const Out r = run ? solve_threads(tree, tasks, first, threads, &tab, ordered, limit) : first;
            fprintf(o, "%d %u %u %llu\n", r.value, r.best, r.status, (unsigned long long)r.nodes);
            hashed += r.nodes;
            continue;
        }
        for (int order = 0; order < norders + plain; order++) {
            const bool bare = order == norders;
            const Out r = run ? solve_serial(tree, tasks, first, bare ? 0 : order, seed, bare ? nullptr : &tab, ordered,
                                             limit)
                              : first;
            fprintf(o, "%d %u %u %llu%s", r.value, r.best, r.status, (unsigned long long)r.nodes,
                    order == norders + plain - 1 ? "\n" : " ");
            if (order == 0) hashed += r.nodes;
            if (bare) unhashed += r.nodes;
        }
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    fclose(o);
    fprintf(stderr,
            "{\"mode\": \"%c\", \"positions\": %zu, \"threads\": %d, \"seconds\": %.6f, \"hashed_nodes\": %llu, "
            "\"unhashed_nodes\": %llu}\n",
            mode, pos.size(), mode == 'b' ? threads : 1, sec, hashed, unhashed);
    return 0;
}
