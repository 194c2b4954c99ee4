// solve_deep_ref.cpp — the reference behind tests/golden/solve_deep/solve_deep.npz: a plain
// recursive alpha-beta over a plain statement of the rules, independent of
// both state machines (solve_core.hpp, solve_order_core.hpp) and of the tree.
//
//   V(pos, mover) = max over the mover's legal moves of -V(child, opponent)
//                 = -V(pos, opponent)                the mover must pass, the opponent can move
//                 = discs(mover) - discs(opponent)   neither can move (no bonus for empties)
//
// Value: every root is solved twice, moves in ascending order and moves in a
// mobility order (fewest opponent moves first in nodes with at least 4
// empties); the two must agree.  Best move: every root move is solved with the
// FULL window, so the lowest maximiser is explicit; its value must be the
// root's.  64 for a forced pass, 255 when the game is over.
//
// build:  g++ -O2 -std=c++17 -fopenmp -o solve_deep_ref tools/diag/solve_deep_ref.cpp
// run:    solve_deep_ref IN OUT [threads=16]
//   IN : one position per line, "<black hex> <white hex> <turn>"
//   OUT: one line per position, "<value> <best_move> <nodes ascending> <nodes ordered>"
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define HOST_IO_NO_CORES  // the positions file's reader alone: no core header is read
#include "host_io.hpp"

typedef uint64_t u64;

static const int kShift[8] = {1, 7, 8, 9, 1, 7, 8, 9};  // the first four to the left, the last four to the right
static const u64 kMask[8] = {0xFEFEFEFEFEFEFEFEull, 0x7F7F7F7F7F7F7F7Full, 0xFFFFFFFFFFFFFFFFull, 0xFEFEFEFEFEFEFEFEull,
                             0x7F7F7F7F7F7F7F7Full, 0xFEFEFEFEFEFEFEFEull, 0xFFFFFFFFFFFFFFFFull, 0x7F7F7F7F7F7F7F7Full};

static inline u64 step(u64 x, int d) { return (d < 4 ? x << kShift[d] : x >> kShift[d]) & kMask[d]; }

// the opponent discs a move on the empty square `bit` turns over
static u64 flips(u64 bit, u64 P, u64 O) {
    u64 all = 0;
    for (int d = 0; d < 8; d++) {
        u64 run = 0, x = step(bit, d);
        while (x & O) {
            run |= x;
            x = step(x, d);
        }
        if (x & P) all |= run;
    }
    return all;
}

static u64 moves(u64 P, u64 O) {
    u64 m = 0;
    for (u64 e = ~(P | O); e; e &= e - 1) {
        const u64 bit = e & -e;
        if (flips(bit, P, O)) m |= bit;
    }
    return m;
}

static int count(u64 x) { return __builtin_popcountll(x); }

struct Counter {
    unsigned long long nodes = 0;
};

// fail-soft negamax; `mobility`: order the moves of nodes with >= 4 empties
static int search(u64 P, u64 O, int alpha, int beta, bool passed, bool mobility, Counter& c) {
    const u64 m = moves(P, O);
    if (m == 0) {
        if (passed || moves(O, P) == 0) return count(P) - count(O);
        c.nodes++;
        return -search(O, P, -beta, -alpha, true, mobility, c);
    }
    struct Cand {
        int key;
        u64 P, O;
    } cand[34];
    int k = 0;
    const bool order = mobility && count(~(P | O)) >= 4;
    for (u64 r = m; r; r &= r - 1) {
        const u64 bit = r & -r, f = flips(bit, P, O);
        cand[k].P = O & ~f;
        cand[k].O = P | f | bit;
        cand[k].key = order ? count(moves(cand[k].P, cand[k].O)) : 0;
        if (order) c.nodes++;
        k++;
    }
    if (order) std::stable_sort(cand, cand + k, [](const Cand& a, const Cand& b) { return a.key < b.key; });
    int best = -65;
    for (int i = 0; i < k; i++) {
        c.nodes++;
        const int v = -search(cand[i].P, cand[i].O, -beta, -(alpha > best ? alpha : best), false, mobility, c);
        if (v > best) best = v;
        if (best >= beta) break;
    }
    return best;
}

struct Job {
    int pos, kind;  // kind 0: the root ascending, 1: the root ordered, 2 + k: root move k, full window
    int value = 0;
    unsigned long long nodes = 0;
};

int main(int argc, char** argv) {
    if (argc < 3) usage(argv[0], "IN OUT [threads]");
    const int threads = argc > 3 ? atoi(argv[3]) : 16;
    if (threads < 1) return 2;
    std::vector<Pos> pos;
    read_positions(argv[1], 0, pos);
    std::vector<Job> jobs;
    for (int i = 0; i < (int)pos.size(); i++) {
        const u64 P = pos[i].mover(), O = pos[i].other();
        if (P & O) return 2;
        jobs.push_back(Job{i, 0});
        jobs.push_back(Job{i, 1});
        for (int k = 0; k < count(moves(P, O)); k++) jobs.push_back(Job{i, 2 + k});
    }
    const long nj = (long)jobs.size();
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long j = 0; j < nj; j++) {
        Job& job = jobs[j];
        const Pos& p = pos[job.pos];
        const u64 P = p.mover(), O = p.other();
        Counter c;
        if (job.kind < 2) {
            job.value = search(P, O, -65, 65, false, job.kind == 1, c);
        } else {
            u64 m = moves(P, O);
            for (int k = 2; k < job.kind; k++) m &= m - 1;
            const u64 bit = m & -m, f = flips(bit, P, O);
            job.value = -search(O & ~f, P | f | bit, -65, 65, false, true, c);
        }
        job.nodes = c.nodes;
    }
    FILE* o = open_or_exit(argv[2], "w");
    long j = 0;
    for (int i = 0; i < (int)pos.size(); i++) {
        const u64 P = pos[i].mover(), O = pos[i].other();
        const Job &asc = jobs[j], &ord = jobs[j + 1];
        j += 2;
        if (asc.value != ord.value) {
            fprintf(stderr, "position %d: ascending %d, ordered %d\n", i, asc.value, ord.value);
            return 3;
        }
        const u64 m = moves(P, O);
        int best = 255;
        if (m == 0) {
            best = moves(O, P) ? 64 : 255;
        } else {
            int top = -65;
            for (u64 r = m; r; r &= r - 1, j++)
                if (jobs[j].value > top) {
                    top = jobs[j].value;
                    best = __builtin_ctzll(r);
                }
            if (top != asc.value) {
                fprintf(stderr, "position %d: value %d, best root move %d\n", i, asc.value, top);
                return 3;
            }
        }
        fprintf(o, "%d %d %llu %llu\n", asc.value, best, asc.nodes, ord.nodes);
    }
    fclose(o);
    return 0;
}
