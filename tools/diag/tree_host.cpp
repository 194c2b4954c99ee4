// tree_host.cpp — the split search's tree (subproc_amd/csrc/tree_core.hpp) and
// the one-lane state machine below it (search_core.hpp) on the host, with a
// plain C++ statement of the rules and plain loads and stores for the atomics.
//
// The expansion, the back-up and the windows are tree_core.hpp's, so the tie
// rule and the empty-window rule of DESIGN.md §15 can be run under
// -fsanitize=address,undefined and compared against tests/search_ref.py before
// any GPU run (the device build differs in the rules, the atomics, the stack
// and in who runs which task when).  Each position's tasks are run in four
// orders: forward, reverse, a seeded shuffle (all with shared bounds), and
// forward with the windows fixed before any task runs ("nothing shared").  All
// four must give the same value, move and status.
//
// build:  g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all
//             -o tools/diag/tree_host_asan tools/diag/tree_host.cpp
// run:    tree_host IN OUT WEIGHTS depth split [nodes_per_position=32768] [node_limit=0] [seed=1] [order=0]
//   order 1: order_core.hpp's ordered machine inside the tasks, root tie rule off
//   IN : one position per line, "<black hex> <white hex> <turn>"
//   WEIGHTS: 36 integers in -128..127, [phase][feature]
//   OUT: one line per position, four times "<value> <best_move> <status> <nodes>"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../subproc_amd/csrc/order_core.hpp"
#include "../../subproc_amd/csrc/tree_core.hpp"
#include "host_io.hpp"
#include "host_rules.hpp"

using otht::Node;
using otht::u32;
using otht::u64;

using HostStack = HostStack9<othm::kFrames>;

struct Out {
    int value;
    u32 best, status;
    u64 nodes;
};

enum Order { kForward, kReverse, kShuffle, kSnapshot };

// tree.hip's expand_kernel and task_kernel for one position, one task at a time
static Out search_one(const Pos& p, int depth, int split, u32 npp, const int* table, u32 limit, Order order,
                      u32 seed, int ordered) {
    if (p.black & p.white) return Out{0, othm::kNoMove, othm::kInvalid, 0};
    std::vector<Node> slab(npp);
    otht::make_node<HostRules>(slab[0], p.mover(), p.other(), -1, othm::kNoMove, depth, otht::kSideRoot);
    const int target = depth - split;
    u32 lvl[otht::kMaxRounds + 2] = {0, 1};
    u32 begin = 0, end = 1;
    int rounds = 0;
    while (rounds < otht::kMaxRounds) {
        u64 total = 0;
        for (u32 i = begin; i < end; i++) total += otht::child_count<HostRules>(slab[i], target);
        if (total == 0 || end + total > npp) break;
        u32 at = end;
        for (u32 i = begin; i < end; i++) {
            const u32 c = otht::child_count<HostRules>(slab[i], target);
            if (c) otht::expand<HostRules>(slab.data(), i, at, c);
            at += c;
        }
        begin = end;
        end += (u32)total;
        lvl[++rounds + 1] = end;
    }
    for (int r = rounds; r >= 1; r--)
        for (u32 i = lvl[r]; i < lvl[r + 1]; i++) {
            const u64 w = slab[i].state;
            if ((slab[i].flags & otht::kFinal) || (slab[i].nchild && otht::count_of(w) == 0))
                otht::fold<HostAtomics>(slab.data(), (u32)slab[i].parent, otht::best_of(w), 0);
        }
    for (u32 i = 0; i < end; i++) slab[i].snap = otht::best_of(slab[i].state);
    std::vector<u32> tasks;
    bool deep = false;
    for (u32 i = 0; i < end; i++)
        if (otht::is_task(slab[i])) {
            tasks.push_back(i);
            deep |= slab[i].rem > othm::kMaxDepth;
        }
    u64 nodes = end - 1;
    if (deep) return Out{0, othm::kNoMove, otht::kNoRoom, nodes};
    Out out{0, othm::kNoMove, othm::kSearched, nodes};
    if (tasks.empty()) {
        otht::root_result<HostAtomics>(slab.data(), out.value, out.best, out.status);
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
        otht::window<HostAtomics>(slab.data(), t, order != kSnapshot, alpha, beta);
        if (alpha >= beta) {
            v = beta;
        } else {
            othm::Lane L;
            HostStack stk;
            otht::start_task(L, slab[t], alpha, beta);
            othm::Order Q;
            othm::order_reset(Q);
            if (ordered)
                while (L.depth >= 0) othm::advance_ordered<HostRules, false>(L, Q, stk, table, limit);
            else
                while (L.depth >= 0) othm::advance<HostRules>(L, stk, table, limit);
            v = L.value;
            lim = L.status == othm::kLimit ? otht::kLimitBit : 0;
            nodes += L.nodes;
        }
        if (emitted) return Out{0, 0, 99, 0};  // the root completed before the last task: a defect
        if (otht::fold_up<HostAtomics>(slab.data(), t, v, lim)) {
            otht::root_result<HostAtomics>(slab.data(), out.value, out.best, out.status);
            emitted = true;
        }
    }
    if (!emitted) return Out{0, 0, 98, 0};  // the root never completed: a defect
    out.nodes = nodes;
    return out;
}

int main(int argc, char** argv) {
    if (argc < 6) usage(argv[0], "IN OUT WEIGHTS depth split [nodes_per_position] [node_limit] [seed] [order]");
    const int depth = atoi(argv[4]), split = atoi(argv[5]);
    const long npp = argc > 6 ? atol(argv[6]) : 32768;
    const u32 limit_arg = argc > 7 ? (u32)strtoul(argv[7], nullptr, 0) : 0u;
    const u32 seed = argc > 8 ? (u32)strtoul(argv[8], nullptr, 0) : 1u;
    const int ordered = argc > 9 ? atoi(argv[9]) : 0;
    if (ordered < 0 || ordered > 1) return 2;
    if (split < 1 || split > otht::kMaxSplit || depth <= split || depth > split + othm::kMaxDepth ||
        npp < otht::kMinNodes || npp > (1 << 24))
        return 2;
    const u32 limit = node_limit(limit_arg);
    int table[othm::kEvalTable];
    read_weights(argv[3], table);
    std::vector<Pos> pos;
    read_positions(argv[1], 0, pos);
    FILE* o = open_or_exit(argv[2], "w");
    for (const Pos& p : pos) {
        for (int order = 0; order < 4; order++) {
            const Out r = search_one(p, depth, split, (u32)npp, table, limit, (Order)order, seed, ordered);
            fprintf(o, "%d %u %u %llu%s", r.value, r.best, r.status, (unsigned long long)r.nodes,
                    order == 3 ? "\n" : " ");
        }
    }
    fclose(o);
    return 0;
}
