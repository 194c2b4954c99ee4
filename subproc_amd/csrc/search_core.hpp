// search_core.hpp — the depth-limited search's state machine, one lane per
// position, written once for the device (search.hip) and the host
// (tools/diag/search_host.cpp).
//
// It is solve_core.hpp's negamax alpha-beta (one step of one position per
// advance() call, the frames below the current one on the stack S, the rules
// from the template parameter R; read that file's header first) with a depth
// horizon:
//   * a frame carries `rem`, the plies left below it.  A move made at rem == 1
//     (or onto the last empty square) gives a LEAF: it is scored on the spot
//     and never pushed, so a search of depth D stores D - 1 frames;
//   * a leaf's score is include/othello_search.h's rule 1 or 2: T * the disc
//     difference when neither side can move there, else the linear eval of the
//     ROOT mover's side (oth_eval's), signed for the frame's mover.  It needs
//     the root side's move mask: the child's own one (the step's R::moves
//     call) when the root side is to move there, one more R::moves otherwise
//     or when the child's mask is empty (the game-over test);
//   * the window is 32 bits wide, (-kInf, kInf) at the root: terminal scores
//     are multiples of T = 2^17 up to 2^23, evals stay below 73,728 < T;
//   * a pass costs no depth (rem unchanged), a frame that finds the game over
//     is worth T * its mover's disc difference.
// Flag kRootSide says whether the frame's mover is the root mover; a push and a
// pass both toggle it.
//
// Window, ties, nodes and the limit are the solver's: fail-hard, strict
// improvement, lowest square first, so the root keeps the LOWEST square among
// its maximisers; nodes = placements + passes; a position whose next node
// would exceed `limit` ends as kLimit.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define OTHM_FN __device__ __forceinline__
#else
#define OTHM_FN inline
#endif

namespace othm {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr int kMaxDepth = 8;              // OTHM_MAX_DEPTH
constexpr int kFrames = kMaxDepth - 1;    // stored frames: rem = D .. 2, the current one is in registers
constexpr int kFields = 9;                // 32-bit words per frame: P, O, M (2 each), alpha, beta, flags + rem
constexpr int kTerminal = 1 << 17;        // OTHM_TERMINAL_SCALE
constexpr int kInf = 1 << 30;

constexpr u32 kSearched = 1, kInvalid = 2, kLimit = 3;  // OTHM_SEARCHED ..
constexpr u32 kNoMove = 255, kPassMove = 64;

constexpr u32 kFresh = 1;     // the frame never had a move and its pass is not checked yet
constexpr u32 kPassed = 2;    // the frame was entered by a pass: its value goes up un-negated
constexpr u32 kRootNew = 4;   // a root whose move mask is not computed yet
constexpr u32 kRootSide = 8;  // the frame's mover is the root mover

// the eval table as the search reads it: oth_eval's int8 [4][9] widened to int
// rows padded to kEvalRow
constexpr int kEvalPhases = 4, kEvalFeatures = 9, kEvalRow = 12;
constexpr int kEvalTable = kEvalPhases * kEvalRow;
// counts() region masks a..h (as othello.hip's kRegionMasks)
constexpr u64 kRegion0 = 0x8100000000000081ull, kRegion1 = 0x4281000000008142ull, kRegion2 = 0x0042000000004200ull,
              kRegion3 = 0x2400810000810024ull, kRegion4 = 0x1800008181000018ull, kRegion5 = 0x003C424242423C00ull,
              kRegion6 = 0x0000240000240000ull, kRegion7 = 0x0000183C3C180000ull;

OTHM_FN void widen_weight(const int8_t* w36, int e, int* table) {
    const int r = e / kEvalRow, c = e % kEvalRow;
    table[e] = c < kEvalFeatures ? (int)w36[r * kEvalFeatures + c] : 0;
}

OTHM_FN u32 eval_shard(u32 discs) { return discs ? ((discs < 64u ? discs : 64u) - 1u) >> 4 : 0u; }

// oth_eval of a position with `discs` discs for the side owning `mine` whose
// legal moves are `mob`
template <class R>
OTHM_FN int eval(const int* table, u64 mine, u64 mob, u32 discs) {
    const int* w = table + kEvalRow * (int)eval_shard(discs);
    int v = R::mul(w[0], R::count(mob));
    v += R::mul(w[1], R::count(mine & kRegion0));
    v += R::mul(w[2], R::count(mine & kRegion1));
    v += R::mul(w[3], R::count(mine & kRegion2));
    v += R::mul(w[4], R::count(mine & kRegion3));
    v += R::mul(w[5], R::count(mine & kRegion4));
    v += R::mul(w[6], R::count(mine & kRegion5));
    v += R::mul(w[7], R::count(mine & kRegion6));
    v += R::mul(w[8], R::count(mine & kRegion7));
    return v;
}

struct Lane {
    u64 P, O, M;
    int alpha, beta;
    u32 flags;
    int rem;       // plies left below the current frame (>= 1)
    int depth;     // of the current frame on the stack; < 0: no position
    u32 nodes;
    u32 root_mv;   // the root move being searched
    u32 best_mv;
    // set when the position ends (depth < 0 again)
    int value;
    u32 status;
};

// a position for the search: mover's discs P, opponent's O (disjoint: the
// caller has checked), `plies` in 1..kMaxDepth
OTHM_FN void start(Lane& L, u64 P, u64 O, int plies) {
    L.P = P;
    L.O = O;
    L.M = 0;
    L.alpha = -kInf;
    L.beta = kInf;
    L.flags = kRootNew | kRootSide;
    L.rem = plies;
    L.depth = 0;
    L.nodes = 0;
    L.root_mv = kNoMove;
    L.best_mv = kNoMove;
    L.value = 0;
    L.status = kSearched;
}

// a root move's child (or the root after its forced pass) as a search of its
// own, for the per-move values of include/othello_moves.h: P's owner is to
// move and is NOT the root mover, so the root-side flag starts clear and every
// leaf below is scored from O's owner's side.  M: P's moves, computed by the
// caller (the kRootNew step would set the flag).  `plies` >= 1 are left below
// this frame; the value comes out from P's owner's side.
OTHM_FN void start_child(Lane& L, u64 P, u64 O, u64 M, int plies) {
    start(L, P, O, plies);
    L.M = M;
    L.flags = M ? 0u : kFresh;
}

OTHM_FN void stop_at_limit(Lane& L) {
    L.depth = -1;
    L.value = 0;
    L.best_mv = kNoMove;
    L.status = kLimit;
}

// a finished child's value, as the current frame's mover sees it
OTHM_FN void apply_score(Lane& L, int score) {
    if (score > L.alpha) {
        L.alpha = score;
        if (L.depth == 0 && !(L.flags & kPassed)) L.best_mv = L.root_mv;
        if (L.alpha >= L.beta) L.M = 0;  // cut-off
    }
}

// a finished child's value with the ROOT TIE RULE of order_core.hpp's header
// (kRootTie; off: apply_score, which is all the unordered machine needs)
template <bool kRootTie>
OTHM_FN void apply_score_tie(Lane& L, int score) {
    if (kRootTie && L.depth == 0 && score == L.alpha && L.root_mv < L.best_mv && L.best_mv < 64u)
        L.best_mv = L.root_mv;  // (the move was searched from alpha - 1: the score is exact)
    apply_score(L, score);
}

// THE PIECES.  advance() below and order_core.hpp's advance_ordered() are ONE
// machine with two choices of the next move.  Each is a head of its own (the
// pops, then which square and the child's boards X, Y) in front of the step's
// one R::moves call and settle_child(), which holds every transition that does
// not depend on the choice: leaf, push, root step, pass, game over.  pop() and
// apply_score_tie() take the root tie rule as a flag.  What keeps the unordered
// kernels as they were is a comparison of their assembly with the build before
// a change, not a second copy of this text.

// POP: the current frame is done (M == 0, checked), its value is alpha
template <bool kRootTie, class S>
OTHM_FN void pop(Lane& L, S& stk) {
    const int score = (L.flags & kPassed) ? L.alpha : -L.alpha;  // for the parent's mover
    if (L.depth == 0) {
        L.depth = -1;
        L.value = -score;
        return;
    }
    L.depth--;
    u32 w;
    stk.load(L.depth, L.P, L.O, L.M, L.alpha, L.beta, w);
    L.flags = w & 0xFFu;
    L.rem = (int)(w >> 8);
    apply_score_tie<kRootTie>(L, score);
}

constexpr int kPopsPerStep = 2;  // as the solver's

// the step's second half.  mv: the head placed a move, (X, Y) is the child and
// cm its mover's moves: a leaf is scored, anything else pushed; `lower` = 1
// widens the child's beta by one (the root tie rule).  !mv: cm settles a new
// root's mask, a pass or the game's end.
template <class R, bool kRootTie, class S>
OTHM_FN void settle_child(Lane& L, S& stk, const int* table, u32 limit, bool mv, u64 X, u64 Y, u64 cm, int lower) {
    const u32 side = L.flags & kRootSide;
    if (mv) {
        if (L.rem <= 1 || ~(X | Y) == 0) {  // a leaf: scored here, nothing pushed
            // side != 0: the root side has just moved (it owns Y) and X's owner is to move
            u64 om = 0;
            if (side || cm == 0) om = R::moves(Y, X);
            int score;
            if ((cm | om) == 0) {
                score = kTerminal * (R::count(Y) - R::count(X));
            } else {
                const int e = eval<R>(table, side ? Y : X, side ? om : cm, (u32)R::count(X | Y));
                score = side ? e : -e;
            }
            apply_score_tie<kRootTie>(L, score);  // (a leaf's score is exact: no window to widen)
            return;
        }
        // (rem <= kMaxDepth at the root and one less per push, so depth <=
        // kFrames - 1 here; the check keeps a defect out of the neighbours' frames)
        if (L.depth >= kFrames) return stop_at_limit(L);
        stk.store(L.depth, L.P, L.O, L.M, L.alpha, L.beta, L.flags | ((u32)L.rem << 8));
        L.depth++;
        L.rem--;
        L.P = X;
        L.O = Y;
        L.M = cm;
        const int a = L.alpha - lower;
        L.alpha = -L.beta;
        L.beta = -a;
        L.flags = (cm ? 0u : kFresh) | (side ^ kRootSide);
    } else if (L.flags & kRootNew) {
        L.M = cm;
        L.flags = (cm ? 0u : kFresh) | kRootSide;
    } else if (cm) {  // CHECK: a pass (no depth spent)
        if (L.nodes >= limit) return stop_at_limit(L);
        L.nodes++;
        L.P = X;
        L.O = Y;
        L.M = cm;
        const int a = L.alpha;
        L.alpha = -L.beta;
        L.beta = -a;
        L.flags = kPassed | (side ^ kRootSide);
        if (L.depth == 0) L.best_mv = kPassMove;
    } else {  // CHECK: game over; the next step pops the frame
        L.flags = side;
        L.alpha = kTerminal * (R::count(L.P) - R::count(L.O));
    }
}

// one step of the lane's search; requires L.depth >= 0.  `table`: the widened
// eval table (kEvalTable ints).  The head: the lowest square of M.
template <class R, class S>
OTHM_FN void advance(Lane& L, S& stk, const int* table, u32 limit) {
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int r = 0; r < kPopsPerStep; r++)
        if (L.depth >= 0 && L.M == 0 && !(L.flags & (kFresh | kRootNew))) pop<false>(L, stk);
    if (L.depth < 0) return;
    u64 X, Y;  // the position to analyse: X to move
    const bool mv = L.M != 0;
    if (mv) {
        if (L.nodes >= limit) return stop_at_limit(L);
        const u32 sq = R::lowest(L.M);
        const u64 bit = 1ull << sq;
        L.M &= L.M - 1;
        const u64 f = R::flips(sq, L.P, L.O);
        X = L.O & ~f;
        Y = L.P | f | bit;
        if (L.depth == 0) L.root_mv = sq;
        L.nodes++;
    } else if (L.flags & kRootNew) {
        X = L.P;
        Y = L.O;
    } else if (L.flags & kFresh) {
        X = L.O;
        Y = L.P;
    } else {
        return;  // a third finished frame in a row: the next step pops it
    }
    const u64 cm = R::moves(X, Y);
    settle_child<R, false>(L, stk, table, limit, mv, X, Y, cm, 0);
}

}  // namespace othm
