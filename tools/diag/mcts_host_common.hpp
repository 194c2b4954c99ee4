// mcts_host_common.hpp — the host side of mcts_core.hpp's walk, shared by
// mcts_host.cpp and mcts_tree_host.cpp: a plain C++ statement of the rules,
// arrays for the tree, loops for the wave's collectives and a plain C++ random
// playout over DESIGN.md §4's draws.
#pragma once
#include <cstring>
#include <vector>

#include "../../subproc_amd/csrc/mcts_core.hpp"
#include "../../subproc_amd/csrc/play_core.hpp"  // DESIGN.md §4's draws: seed_state, game_key, Rng
#include "host_io.hpp"
#include "host_rules.hpp"

typedef uint64_t u64;
typedef uint32_t u32;

// the IN file of both programs: positions with `extras` extra columns (a line
// short of them is passed over), and the table as lines "L <float32 bits hex>"
static void read_trees(const char* path, int extras, std::vector<Pos>& pos, std::vector<float>& table) {
    FILE* in = open_or_exit(path, "r");
    char line[4096];
    while (fgets(line, sizeof line, in)) {
        unsigned bits;
        Pos p;
        if (sscanf(line, "L %x", &bits) == 1) {
            float f;
            memcpy(&f, &bits, 4);
            table.push_back(f);
        } else if (parse_position(line, p) >= 3 + extras) {
            pos.push_back(p);
        }
    }
    fclose(in);
}

struct Rules : HostRules {
    static u32 kth(u64 m, u32 k) {
        for (; k; k--) m &= m - 1;
        return lowest(m);
    }
};

// one uniformly random game from (P to move, O); the final disc difference from O's side
static int play_out(u64 P, u64 O, u64 key, u64* plies) {
    othp::Rng rng;
    rng.init(key);
    bool flipped = false;  // P is the leaf's other side
    for (;;) {
        const u64 legal = Rules::moves(P, O);
        if (legal) {
            const u32 sq = Rules::kth(legal, rng.pick((u32)Rules::count(legal)));
            const u64 f = Rules::flips(sq, P, O);
            P |= f | (1ull << sq);
            O &= ~f;
        } else if (Rules::moves(O, P) == 0) {
            break;
        }
        ++*plies;  // (a pass is an env-step too)
        const u64 x = P;
        P = O;
        O = x;
        flipped = !flipped;
    }
    const int d = Rules::count(O) - Rules::count(P);
    return flipped ? -d : d;
}

struct HostTree {
    std::vector<u64> P, O;
    std::vector<u32> nn, ss, link_;
    std::vector<int> dd;
    explicit HostTree(u32 M) : P(M), O(M), nn(M), ss(M), link_(M), dd(M) {}
    void pos(u32 v, u64& p, u64& o) const { p = P.at(v), o = O.at(v); }
    void set_pos(u32 v, u64 p, u64 o) { P.at(v) = p, O.at(v) = o; }
    void visits_wins(u32 v, u32& n, u32& s) const { n = nn.at(v), s = ss.at(v); }
    u32 n(u32 v) const { return nn.at(v); }
    int d(u32 v) const { return dd.at(v); }
    u32 link(u32 v) const { return link_.at(v); }
    void set_stats(u32 v, u32 n, u32 s, int d) { nn.at(v) = n, ss.at(v) = s, dd.at(v) = d; }
    void set_link(u32 v, u32 l) { link_.at(v) = l; }
    void add_stats(u32 v, u32 n, u32 s, int d) { nn.at(v) += n, ss.at(v) += s, dd.at(v) += d; }
    void mark(u32 v) { nn.at(v) += 1; }  // the wide search's two halves of add_stats (mcts_wide_core.hpp)
    void add_result(u32 v, u32 s, int d) { ss.at(v) += s, dd.at(v) += d; }
    void sync() const {}
};

struct HostWave {
    u32 path[othu::kPathEntries];
    u64 plies = 0;       // env-steps of the playouts (the bench's count)
    u64 wave_plies = 0;  // the longest game of every iteration: what 64 games in lockstep wait for
    template <class F>
    void each(u32 count, F f) const {
        for (u32 k = 0; k < count; k++) f(k);
    }
    template <class F>
    u32 pick(u32 cnt, F f) const {
        u32 best = 0;
        float best_score = 0;
        for (u32 k = 0; k < cnt; k++) {
            bool fresh = false;
            float sc = 0;
            f(k, fresh, sc);
            if (fresh) return k;
            if (k == 0 || othu::better(sc, k, best_score, best)) best = k, best_score = sc;
        }
        return best;
    }
    void path_set(u32 k, u32 v) {
        if (k < othu::kPathEntries) path[k] = v;
    }
    u32 path_get(u32 k) const { return path[k < othu::kPathEntries ? k : 0]; }
    void sync() const {}
    // the re-rooting's prefix sums (mcts_core.hpp's compact())
    u32 scan_words[othu::kLanes], scan_sums[othu::kLanes];
    template <class F>
    u32 scan(u32 count, F f) {
        u32 total = 0;
        for (u32 k = 0; k < count; k++) {
            u32 word = 0, weight = 0;
            f(k, word, weight);
            scan_words[k] = word;
            scan_sums[k] = total;
            total += weight;
        }
        return total;
    }
    u32 scan_word(u32 k) const { return scan_words[k]; }
    u32 scan_below(u32 k) const { return scan_sums[k]; }
    void playout(u64 P, u64 O, u64 id0, u64 seed_state, u32& W, int& D) {
        W = 0, D = 0;
        u64 longest = 0;
        for (u32 j = 0; j < othu::kLanes; j++) {
            u64 len = 0;
            const int dp = play_out(P, O, othp::game_key(seed_state, id0 + j), &len);
            W += othu::half_points(dp);
            D += dp;
            plies += len;
            if (len > longest) longest = len;
        }
        wave_plies += longest;
    }
};
