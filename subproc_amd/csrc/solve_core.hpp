// solve_core.hpp — the exact endgame solver's state machine, one lane per
// position, written once for the device (solve.hip) and the host
// (tools/diag/solve_host.cpp).
//
// The search is a negamax alpha-beta without recursion: advance() does ONE
// step of one position, so that the lanes of a wave, each at its own depth of
// its own tree, run the same instructions.  The rules come from the template
// parameter R (the device: bitboard.hpp's moves() / flips_carry(); the host: a
// plain C++ version), the frames below the current one from the stack S
// (the device: an LDS array indexed [depth][field][lane]; the host: an array).
//
// Frame = the mover's discs P, the opponent's O, the moves M not yet tried,
// the window (alpha, beta) seen by the frame's mover, and flags.  The current
// frame lives in registers (Lane); push stores it, pop loads its parent: one
// stack access per step.  A step is one of
//   MOVE   M != 0: take M's lowest square, place it (R::flips), analyse the
//          child (R::moves) and push; a child without an empty square is
//          scored on the spot (nothing pushed);
//   ROOT   a root just loaded: its move mask (R::moves);
//   CHECK  a frame that never had a move: the opponent's moves (R::moves).
//          Some: a pass, the frame becomes the opponent's (same depth, window
//          negated, flag PASSED).  None: game over, the value is the disc
//          difference (no bonus for empty squares), then as POP;
//   POP    M == 0: hand the frame's value to its parent.
// MOVE, ROOT and CHECK share the one R::moves call of the step; up to two
// POPs are made at the start of the step that makes the next move.
//
// Window and ties: fail-hard, alpha is the running maximum, a score replaces
// it only when strictly greater.  The root starts at (-65, 65), so every root
// move's first equal-or-better rival fails low and the move kept is the LOWEST
// square among the maximisers (moves are taken lowest bit first everywhere).
// start() may be given a narrower root window (alpha, beta): the same machine
// then keeps the lowest square among the moves that reach beta when the value
// does, and no move (kNoMove) when no move beats alpha.  A finished game is
// scored as it is, whatever the window, so a root's value is clamped into its
// window by whoever emits it (clamp_to_window).
//
// Nodes = MOVE steps (placements) + passes.  A position whose next node would
// exceed `limit` ends as kLimit; every step pops a frame or makes a node (or
// is one of a position's two first steps), and pops are at most one per node,
// so a position's steps are bounded by 2 * limit + 2.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define OTHS_FN __device__ __forceinline__
#else
#define OTHS_FN inline
#endif

namespace oths {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr int kMaxEmpties = 12;           // OTHS_MAX_EMPTIES
// frames kept on the stack: the current one is in registers and a child with
// no empty square is never pushed, so a root of E empties stores depths 0..E-2
constexpr int kFrames = kMaxEmpties - 1;
constexpr int kFields = 7;                // 32-bit words per frame: P, O, M (2 each), packed window + flags

constexpr u32 kSkipped = 0, kSolved = 1, kInvalid = 2, kLimit = 3;  // OTHS_SKIPPED ..
constexpr u32 kBadWindow = 5;             // OTHS_BADWINDOW (4 is the split solver's OTHE_NOROOM)
constexpr int kInf = 65;                  // the full root window is (-kInf, kInf)
constexpr u32 kNoMove = 255, kPassMove = 64;

constexpr u32 kFresh = 1;   // the frame never had a move and its pass is not checked yet
constexpr u32 kPassed = 2;  // the frame was entered by a pass: its value goes up un-negated
constexpr u32 kRootNew = 4; // a root whose move mask is not computed yet

struct Lane {
    u64 P, O, M;
    int alpha, beta;
    u32 flags;
    int depth;     // of the current frame; < 0: no position
    u32 nodes;
    u32 root_mv;   // the root move being searched
    u32 best_mv;
    // set when the position ends (depth < 0 again)
    int value;
    u32 status;
};

OTHS_FN u32 pack(int alpha, int beta, u32 flags) {
    return (u32)(alpha & 0xFF) | ((u32)(beta & 0xFF) << 8) | (flags << 16);
}

// a position for the search: mover's discs P, opponent's O (disjoint, at most
// kMaxEmpties empty squares: the caller has checked both) and the root window
// -kInf <= alpha < beta <= kInf (window_ok: the caller has checked that too)
OTHS_FN void start(Lane& L, u64 P, u64 O, int alpha = -kInf, int beta = kInf) {
    L.P = P;
    L.O = O;
    L.M = 0;
    L.alpha = alpha;
    L.beta = beta;
    L.flags = kRootNew;
    L.depth = 0;
    L.nodes = 0;
    L.root_mv = kNoMove;
    L.best_mv = kNoMove;
    L.value = 0;
    L.status = kSolved;
}

OTHS_FN void stop_at_limit(Lane& L) {
    L.depth = -1;
    L.value = 0;
    L.best_mv = kNoMove;
    L.status = kLimit;
}

// a finished child's value, as the current frame's mover sees it
OTHS_FN void apply_score(Lane& L, int score) {
    if (score > L.alpha) {
        L.alpha = score;
        if (L.depth == 0 && !(L.flags & kPassed)) L.best_mv = L.root_mv;
        if (L.alpha >= L.beta) L.M = 0;  // cut-off
    }
}

// POP: the current frame is done (M == 0, checked), its value is alpha
template <class S>
OTHS_FN void pop(Lane& L, S& stk) {
    const int score = (L.flags & kPassed) ? L.alpha : -L.alpha;  // for the parent's mover
    if (L.depth == 0) {
        L.depth = -1;
        L.value = -score;
        return;
    }
    L.depth--;
    u32 w;
    stk.load(L.depth, L.P, L.O, L.M, w);
    L.alpha = (int)(int8_t)(w & 0xFF);
    L.beta = (int)(int8_t)((w >> 8) & 0xFF);
    L.flags = w >> 16;
    apply_score(L, score);
}

// the pops a step makes before its move: a pop is a stack load and a compare,
// a move some three hundred instructions, so finished frames are taken off in
// the step that makes the next move and do not cost a step of their own (two
// cover nearly every case; a third waits for the next step)
constexpr int kPopsPerStep = 2;

// THE PIECES.  advance() below and solve_order_core.hpp's advance_ordered() are
// ONE machine with two choices of the next move.  Each is a head of its own
// (the pops, then which square and the child's boards X, Y) in front of the
// step's one R::moves call and settle_child(), which holds every transition
// that does not depend on the choice: board full, push, root step, pass, game
// over.  What keeps solve_kernel as it was is a comparison of its assembly with
// the build before a change, not a second copy of this text.

// the step's second half.  mv: the head placed a move, (X, Y) is the child and
// cm its mover's moves; !mv: cm settles a new root's mask, a pass or the game's end
template <class R, class S>
OTHS_FN void settle_child(Lane& L, S& stk, u32 limit, bool mv, u64 X, u64 Y, u64 cm) {
    if (mv) {
        if (~(X | Y) == 0) {  // board full: the child's value for us, nothing pushed
            apply_score(L, R::count(Y) - R::count(X));
            return;
        }
        // (a root has at most kMaxEmpties empties, so depth <= kFrames - 1
        // here; the check keeps a defect out of the neighbours' frames)
        if (L.depth >= kFrames) return stop_at_limit(L);
        stk.store(L.depth, L.P, L.O, L.M, pack(L.alpha, L.beta, L.flags));
        L.depth++;
        L.P = X;
        L.O = Y;
        L.M = cm;
        const int a = L.alpha;
        L.alpha = -L.beta;
        L.beta = -a;
        L.flags = cm ? 0u : kFresh;
    } else if (L.flags & kRootNew) {
        L.M = cm;
        L.flags = cm ? 0u : kFresh;
    } else if (cm) {  // CHECK: a pass
        if (L.nodes >= limit) return stop_at_limit(L);
        L.nodes++;
        L.P = X;
        L.O = Y;
        L.M = cm;
        const int a = L.alpha;
        L.alpha = -L.beta;
        L.beta = -a;
        L.flags = kPassed;
        if (L.depth == 0) L.best_mv = kPassMove;
    } else {  // CHECK: game over; the next step pops the frame
        L.flags = 0;
        L.alpha = R::count(L.P) - R::count(L.O);
    }
}

// one step of the lane's search; requires L.depth >= 0.  The head: the lowest
// square of M.
template <class R, class S>
OTHS_FN void advance(Lane& L, S& stk, u32 limit) {
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int r = 0; r < kPopsPerStep; r++)
        if (L.depth >= 0 && L.M == 0 && !(L.flags & (kFresh | kRootNew))) pop(L, stk);
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
    settle_child<R>(L, stk, limit, mv, X, Y, cm);
}

// what a position is before any search (kSolved: search it); empties = the
// number of its empty squares
OTHS_FN u32 classify(u64 black, u64 white, int empties, int max_empties) {
    if (black & white) return kInvalid;
    return empties > max_empties ? kSkipped : kSolved;
}


OTHS_FN bool window_ok(int alpha, int beta) { return alpha >= -kInf && alpha < beta && beta <= kInf; }

// a root's value as its caller sees it: the machine is fail-hard but for the
// finished games, which are scored exactly
OTHS_FN int clamp_to_window(int v, int alpha, int beta) { return v < alpha ? alpha : v > beta ? beta : v; }

}  // namespace oths
