// game_loop.hpp — what the game kernels (play.hip's, budget.hip's and
// play_solve.hip's first phase) share, stated once: a game's move record and
// its outputs, the persistent loop that plays the games, and the host side of
// their entry points (the check and the fill of the common arguments).
// Everything device-side is force-inlined into the kernels; it reads the
// kernel's own argument struct (PlayArgs, BudgetPlayArgs, ZoneArgs: the same
// names for what they share, layouts of their own: one struct for the three
// changes the kernels' code).
#pragma once
#include "../../include/othello.h"
#include "../../include/othello_order.h"
#include "../../include/othello_play.h"
#include "../../include/othello_search.h"
#include "budget_core.hpp"
#include "device_common.hpp"
#include "play_core.hpp"

namespace othp {

// a game's move record: the row starts 255-padded, a move is one byte store
struct MoveRecord {
    uint8_t* row;  // NULL: no record
    __device__ __forceinline__ void pad() const {
        if (!row) return;
#pragma unroll
        for (int q = 0; q < OTH_MOVES_STRIDE / 16; q++) reinterpret_cast<uint4*>(row)[q] = make_uint4(~0u, ~0u, ~0u, ~0u);
    }
    __device__ __forceinline__ void move(othm::u32 ply, othm::u32 code) const {
        if (row && ply < (othm::u32)OTH_MOVES_STRIDE) row[ply] = (uint8_t)code;
    }
};

// game g has ended (G.status says how): its outputs, and the histogram's bins
// if it was played to its end
template <class Args>
__device__ __forceinline__ void emit(const Args& a, othm::u64 g, const Game& G) {
    const othm::u64 bl = black_of(G), wh = white_of(G);
    const int d = G.status == othm::kInvalid ? 0 : __popcll(bl) - __popcll(wh);
    if (a.a_black) a.a_black[g] = (uint8_t)G.a_black;
    if (a.final_boards) reinterpret_cast<ulonglong2*>(a.final_boards)[g] = make_ulonglong2(bl, wh);
    if (a.diff) a.diff[g] = (int8_t)d;
    if (a.plies) a.plies[g] = (uint8_t)G.ply;
    if (a.status) a.status[g] = (uint8_t)G.status;
    if (a.nodes) a.nodes[g] = G.nodes;
    if (a.hist && G.status == othm::kSearched) {
        atomicAdd(&a.hist[d + 64], 1ull);
        atomicAdd(&a.hist[d > 0 ? 129 : (d < 0 ? 130 : 131)], 1ull);
        atomicAdd(&a.hist[132], (unsigned long long)G.ply);
    }
}

// the parking step of the kernels that have none
struct NoPark {};

// THE GAME LOOP: the persistent loop of every game kernel, one wave per block
// of kBlock lanes, one lane per game.  The lanes refill from the work word
// (device_common.hpp's take()) at game granularity; a live lane takes one step
// of play_core.hpp's advance(), or of budget_core.hpp's advance_play() where
// the searches go by node budget (kBudget; Args then has `budgets`).
// kOrdered: order_core.hpp's machine.  kPark: a game whose turn begins inside
// the zone leaves as kParked and goes to park(a, game, G) in place of emit().
template <int kBlock, bool kOrdered, bool kBudget, bool kPark = false, class Args, class Park = NoPark>
__device__ __forceinline__ void game_body(const Args& a, Park park = Park()) {
    using othd::DeviceRules;
    using othm::u32;
    using othm::u64;
    __shared__ u32 frames[othm::kFrames * othm::kFields * kBlock];
    __shared__ int tables[2 * othm::kEvalTable];
    const u32 lane = threadIdx.x;
    if (lane < (u32)othm::kEvalTable) {
        othm::widen_weight(a.w[0], (int)lane, tables);
        othm::widen_weight(a.w[1], (int)lane, tables + othm::kEvalTable);
    }
    __syncthreads();
    othd::LdsStack9<kBlock> stk{frames + lane};
    othm::Lane L;
    L.depth = -1;
    othm::Order Q;  // (unused, and gone, when !kOrdered)
    othm::order_reset(Q);
    othb::Deepen D;  // (unused, and gone, when !kBudget)
    D.d = 0;
    Game G;
    G.live = false;
    MoveRecord rec{nullptr};
    u64 idx = 0;
    bool exhausted = false;  // the lane has made its failing request
    for (;;) {
        const bool idle = !G.live;
        const bool want = idle && !exhausted;
        const u64 wantm = __ballot(want);
        const u64 busym = __ballot(!idle);
        if ((wantm | busym) == 0) break;
        const u64 cnt = (u64)__popcll(wantm);
        if (wantm != 0 && ((int)cnt >= othd::kRefillMin || busym == 0)) {
            const u64 g = othd::take(a.work, a.total, wantm, cnt, lane);
            if (want) {
                if (g >= a.n) {
                    exhausted = true;
                } else {
                    u64 black = kOpenBlack, white = kOpenWhite;
                    bool white_to_move = false;
                    if (a.start) {
                        const ulonglong2 b = reinterpret_cast<const ulonglong2*>(a.start)[g];
                        black = b.x;
                        white = b.y;
                        white_to_move = a.start_turn && a.start_turn[g] == OTH_WHITE;
                    }
                    rec.row = a.moves ? a.moves + g * OTH_MOVES_STRIDE : nullptr;
                    rec.pad();
                    begin(G, L, a.match, game_key(a.seed_state, a.game_id0 + g), black, white, white_to_move);
                    D.d = 0;
                    idx = g;
                    if (!G.live) emit(a, g, G);  // overlapping boards
                }
            }
        }
        if (G.live) {
            if constexpr (kBudget)
                othb::advance_play<DeviceRules, kOrdered, kPark>(G, L, Q, D, stk, tables, a.match, a.budgets, rec);
            else
                advance<DeviceRules, kOrdered, kPark>(G, L, Q, stk, tables, a.match, rec);
            if (!G.live) {
                if constexpr (kPark) {
                    if (G.status == kParked)
                        park(a, idx, G);
                    else
                        emit(a, idx, G);
                } else {
                    emit(a, idx, G);
                }
            }
        }
    }
}

// THE HOST SIDE of the game entry points (otho_play_ordered, othb_play,
// othx_play).  What they check alike: the arguments every one of them takes.
// The budgets, the range of exact_empties / solve_empties and the scratch stay
// with the entry points.
inline bool game_args_ok(int order, int64_t n, const uint64_t* work, const int8_t* weights_a, const int8_t* weights_b,
                         int depth_a, int depth_b, int n_rand_a, int n_rand_b) {
    return order >= 0 && order <= OTHO_MAX_ORDER && n >= 0 && work && weights_a && weights_b && depth_a >= 1 &&
           depth_a <= OTHM_MAX_DEPTH && depth_b >= 1 && depth_b <= OTHM_MAX_DEPTH && n_rand_a >= 0 && n_rand_b >= 0;
}

// What they fill alike: every member the three argument structs share.  lanes:
// the grid's, for `total`; exact_empties: othx_play passes its solve_empties.
template <class Args>
inline void fill_game(Args& a, const uint64_t* start, const uint8_t* start_turn, uint64_t seed, uint64_t game_id0,
                      const int8_t* weights_a, const int8_t* weights_b, int depth_a, int depth_b, int exact_empties,
                      int n_rand_a, int n_rand_b, int swap_colours, uint32_t node_limit, uint8_t* a_black,
                      uint64_t* final_boards, int8_t* diff, uint8_t* plies, uint8_t* moves, uint8_t* status,
                      uint64_t* nodes, int64_t* hist, uint64_t* work, int64_t n, int64_t lanes) {
    a.start = start;
    a.start_turn = start_turn;
    a.a_black = a_black;
    a.final_boards = final_boards;
    a.diff = diff;
    a.plies = plies;
    a.moves = moves;
    a.status = status;
    a.nodes = nodes;
    a.hist = reinterpret_cast<unsigned long long*>(hist);
    a.work = reinterpret_cast<unsigned long long*>(work);
    a.n = (othm::u64)n;
    a.total = (othm::u64)n + (othm::u64)lanes;
    a.seed_state = seed_state(seed);
    a.game_id0 = game_id0;
    a.match.depth[0] = depth_a;
    a.match.depth[1] = depth_b;
    a.match.n_rand[0] = (othm::u32)std::min(n_rand_a, OTHP_MAX_RANDOM);
    a.match.n_rand[1] = (othm::u32)std::min(n_rand_b, OTHP_MAX_RANDOM);
    a.match.exact_empties = exact_empties;
    a.match.limit = node_limit ? node_limit : OTHM_DEFAULT_NODE_LIMIT;
    a.match.swap = swap_colours != 0;
    for (int k = 0; k < OTH_EVAL_WEIGHTS; k++) {
        a.w[0][k] = weights_a[k];
        a.w[1][k] = weights_b[k];
    }
}

}  // namespace othp
