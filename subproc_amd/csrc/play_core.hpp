// play_core.hpp — whole games between two searching players, one lane per
// game: the game driver around search_core.hpp's advance(), written once for
// the device (play.hip) and the host (tools/diag/play_host.cpp).
//
// A lane is either inside a search (othm::Lane::depth >= 0: the caller calls
// othm::advance()) or between two searches (depth < 0: the caller calls step()
// below).  step() is the one more transition of the search's machine: it plays
// the move the last step or the finished search decided, records it, swaps the
// sides, analyses the new position and settles, in include/othello_play.h's
// order, game over / pass / coin / single move; otherwise it starts the next
// root with the new mover's depth.  One step() makes at most one ply, so a
// lane between searches costs its wave one flips and two move masks per
// iteration, like a search step.
//
// The rules come from the template parameter R (search_core.hpp's: moves,
// flips, lowest, count).  The draws are othello.hip's: the key
// mixer, the 32-bit LCG, pick = the high word of draw * n, and the k-th set bit
// of the move mask in puttables order; they are restated here, as
// search_core.hpp restates the eval, so the existing kernels compile from the
// text they always had.
#pragma once
#include <stdint.h>

#include "order_core.hpp"
#include "search_core.hpp"

namespace othp {

using othm::u32;
using othm::u64;

constexpr u64 kGolden64 = 0x9E3779B97F4A7C15ull;
constexpr u32 kLcgMul = 0x915F77F5u;
constexpr u64 kOpenBlack = 0x0000000810000000ull, kOpenWhite = 0x0000001008000000ull;
constexpr u32 kMaxBudget = 10;     // N_RAND_HAND_UNTIL
constexpr u32 kMovesStride = 128;  // OTH_MOVES_STRIDE
constexpr u32 kMaxPlies = 255;     // a game stops here: plies is a byte
constexpr u32 kPassMove = 64;

#ifdef __HIPCC__
#define OTHP_HOST_FN __host__ __device__ __forceinline__  // the launch computes the seed's state
#else
#define OTHP_HOST_FN inline
#endif

OTHP_HOST_FN u64 mix64(u64 z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
OTHP_HOST_FN u64 seed_state(u64 seed) { return mix64(seed + kGolden64); }
OTHM_FN u64 game_key(u64 S, u64 g) { return mix64(S + g * kGolden64); }

struct Rng {
    u32 state, inc;
    OTHM_FN void init(u64 key) {
        state = (u32)key;
        inc = (u32)(key >> 32) | 1u;
    }
    OTHM_FN u32 pick(u32 n) {
        state = state * kLcgMul + inc;
        return (u32)(((u64)state * (u64)n) >> 32);
    }
};

// the k-th (0-based) set bit of m, k < popcount(m)
template <class R>
OTHM_FN u32 kth_set_bit(u64 m, u32 k) {
    for (; k; k--) m &= m - 1;
    return R::lowest(m);
}

// the launch's rule arguments; index 0 is player A, 1 is player B
struct Match {
    int depth[2];
    u32 n_rand[2];  // capped at kMaxBudget
    int exact_empties;
    u32 limit;      // nodes per search
    bool swap;
};

constexpr u32 kMoveNone = 255;    // Game::next: nothing decided, analyse the position
constexpr u32 kMoveSearch = 254;  // Game::next: the move is the running search's
constexpr u32 kParked = 0;        // Game::status of a game step<R, true>() took out of play: no output carries it

struct Game {
    u64 P, O;         // the mover's discs, the other side's
    Rng rng;
    u32 ply;
    u32 rem, rem_other;  // random budgets left: the mover's, the other side's
    bool mover_black, a_black;
    bool live;        // false: no game (not begun, or ended: see status)
    u32 next;         // the move step() plays first, or kMoveNone / kMoveSearch
    u32 status;       // othm::kSearched / kInvalid / kLimit, set when the game ends
    u64 nodes;        // the game's searches' nodes
};

// 0: the mover is player A, 1: player B (the index of its table and depth)
OTHM_FN u32 mover_player(const Game& G) { return G.mover_black == G.a_black ? 0u : 1u; }

// (both boards read before the choice: a choice between the two fields' addresses
// would keep the device's Game out of registers)
OTHM_FN u64 black_of(const Game& G) {
    const u64 p = G.P, o = G.O;
    return G.mover_black ? p : o;
}
OTHM_FN u64 white_of(const Game& G) {
    const u64 p = G.P, o = G.O;
    return G.mover_black ? o : p;
}

// game `key` from black / white with `white_to_move`: the colour draw and the
// budgets.  Overlapping boards end the game at once as kInvalid, no draw made.
OTHM_FN void begin(Game& G, othm::Lane& L, const Match& m, u64 key, u64 black, u64 white, bool white_to_move) {
    L.depth = -1;
    G.P = white_to_move ? white : black;
    G.O = white_to_move ? black : white;
    G.mover_black = !white_to_move;
    G.a_black = true;
    G.ply = 0;
    G.rem = G.rem_other = 0;
    G.next = kMoveNone;
    G.nodes = 0;
    G.status = othm::kSearched;
    G.rng.init(key);
    G.live = (black & white) == 0;
    if (!G.live) {
        G.status = othm::kInvalid;
        return;
    }
    G.a_black = !(m.swap && G.rng.pick(2) == 1u);
    // Black's, White's (selects, not a lane-dependent index into the launch's arguments)
    const u32 rb = G.a_black ? m.n_rand[0] : m.n_rand[1], rw = G.a_black ? m.n_rand[1] : m.n_rand[0];
    G.rem = white_to_move ? rw : rb;
    G.rem_other = white_to_move ? rb : rw;
}

OTHM_FN void hand_over(Game& G) {
    const u32 r = G.rem;
    G.rem = G.rem_other;
    G.rem_other = r;
    G.mover_black = !G.mover_black;
    G.ply++;
}

// One step of a live game whose lane is not searching (L.depth < 0).  `out`
// receives every move: out.move(ply, code).  The game has ended when G.live is
// false on return; a search has started when L.depth >= 0.
// kPark (play_solve.hip's first phase): a game whose turn begins with at most
// m.exact_empties empty squares is not played on: it leaves as kParked, no draw
// of that turn made, for the exact endgame (play_solve_core.hpp) to take up.
template <class R, bool kPark = false, class Out>
OTHM_FN void step(Game& G, othm::Lane& L, const Match& m, Out& out) {
    u32 mv = G.next;
    if (mv == kMoveSearch) {
        G.nodes += L.nodes;
        if (L.status == othm::kLimit) {
            G.status = othm::kLimit;
            G.live = false;
            return;
        }
        mv = L.best_mv;
    }
    G.next = kMoveNone;
    if (G.ply >= kMaxPlies) {  // (not reached from disjoint boards: at most 60 placements and 61 passes)
        G.status = othm::kLimit;
        G.live = false;
        return;
    }
    if (mv < 64u) {
        const u64 f = R::flips(mv, G.P, G.O);
        const u64 np = G.O & ~f;
        G.O = G.P | f | (1ull << mv);
        G.P = np;
        out.move(G.ply, mv);
        hand_over(G);
    }
    if constexpr (kPark) {
        if (64 - R::count(G.P | G.O) <= m.exact_empties) {
            G.status = kParked;
            G.live = false;
            return;
        }
    }
    const u64 own = R::moves(G.P, G.O);
    if (own == 0) {
        if (R::moves(G.O, G.P) == 0) {  // neither side can move: the game is over
            G.live = false;
            return;
        }
        if (G.rem) (void)G.rng.pick(G.rem);  // the passer's turn draws its coin too
        const u64 t = G.P;
        G.P = G.O;
        G.O = t;
        out.move(G.ply, kPassMove);
        hand_over(G);
        return;  // the next step analyses the other side's turn
    }
    const u32 cnt = (u32)R::count(own);
    if (G.rem && G.rng.pick(G.rem) == 0u) {  // the coin: a random legal move
        G.next = kth_set_bit<R>(own, G.rng.pick(cnt));
        G.rem--;
        return;
    }
    if (cnt == 1u) {
        G.next = R::lowest(own);
        return;
    }
    const int empties = 64 - R::count(G.P | G.O);
    int d = mover_player(G) ? m.depth[1] : m.depth[0];
    if (empties <= m.exact_empties && empties > d) d = empties;
    othm::start(L, G.P, G.O, d);
    // the root's move mask is known: enter the search past its kRootNew step
    L.M = own;
    L.flags = othm::kRootSide;
    G.next = kMoveSearch;
}

// One step of a live game's lane: of its search, and of the game when that
// leaves the lane without one.  `tables`: A's widened eval table, then B's
// (2 x othm::kEvalTable ints); each search reads its mover's.  kOrdered: both
// players search with order_core.hpp's machine (the games' moves are the same);
// Q is the lane's scoring state, reset with every new root, and unused otherwise.
template <class R, bool kOrdered, bool kPark = false, class S, class Out>
OTHM_FN void advance(Game& G, othm::Lane& L, othm::Order& Q, S& stk, const int* tables, const Match& m, Out& out) {
    if (L.depth >= 0) {
        if constexpr (kOrdered)
            othm::advance_ordered<R, true>(L, Q, stk, tables + othm::kEvalTable * (int)mover_player(G), m.limit);
        else
            othm::advance<R>(L, stk, tables + othm::kEvalTable * (int)mover_player(G), m.limit);
    }
    if (L.depth < 0) {
        step<R, kPark>(G, L, m, out);
        if constexpr (kOrdered) othm::order_reset(Q);
    }
}

}  // namespace othp
