// perft_core.hpp — perft's counting machine (include/othello_perft.h), one lane
// per task, written once for the device (perft.hip) and the host
// (tools/diag/perft_host.cpp), and the task word the two share.
//
// N(pos, s, d), the number of move paths of length d — a pass is a ply, a
// finished game is one path — is summed without recursion: advance() does ONE
// step of one task, so that the lanes of a wave, each at its own depth of its
// own tree, run the same instructions.  The rules come from the template
// parameter R, the frames below the current one from the stack S, as in
// solve_core.hpp.
//
// Frame = the mover's discs P, the opponent's O, the moves M not yet tried: 6
// words.  The plies left are not stored: every frame has one fewer than the
// frame below it (a pass pushes a frame too).  The lane keeps the running
// count (u64), the plies left of the current frame and its node counter in
// registers.  A step is zero to two POPs and then one ANALYSIS of a position
// (X to move against Y, r plies left), which is
//   MOVE   M != 0: the child after M's lowest square (R::flips), r = rem - 1;
//   ROOT   a task just started: the task itself, r = rem;
//   CHECK  a frame that never had a move: the same board with the other side
//          to move, r = rem - 1 (the pass is a ply).
// The analysis is the step's one R::moves call and counts one node:
//   r == 1    the last ply, counted in bulk: the count grows by the number of
//             moves, or by 1 where there is none (a pass to a leaf or a
//             finished game).  No flip is computed, nothing is pushed;
//   moves     the analysed position becomes the current frame (pushed over its
//             parent but at the root);
//   none, in CHECK: the game is over, one path;
//   none      the position becomes the current frame, marked for CHECK.
// Only positions with r >= 2 get a frame, so a task of D plies stores at most
// D - 2 frames.
//
// Nodes = analyses.  A task whose next analysis would exceed `limit` ends as
// kLimit; every step pops a frame or makes an analysis, and pops are at most
// one per analysis, so a task's steps are bounded by 2 * limit + 2.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define OTHC_FN __device__ __forceinline__
#else
#define OTHC_FN inline
#endif

namespace othc {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr int kMaxDepth = 14;          // OTHC_MAX_DEPTH
constexpr int kFrames = kMaxDepth - 1; // 12 are reached (above); the header's figure
constexpr int kFields = 6;             // 32-bit words per frame: P, O, M

constexpr u32 kCounted = 1, kInvalid = 2, kLimit = 3, kBadDepth = 7;  // OTHC_COUNTED ..

constexpr u32 kFresh = 1;    // the frame never had a move and its pass is not checked yet
constexpr u32 kRootNew = 2;  // a task whose move mask is not computed yet

// THE TASK WORD: position index | root square | plies left | over
constexpr int kSqShift = 24, kRemShift = 31, kOverShift = 35;
constexpr u64 kIndexMask = (1ull << kSqShift) - 1;  // OTHC_MAX_TASKS positions
constexpr u32 kSqPass = 64, kSqNone = 127;          // OTH_PASS; not below a root move yet

OTHC_FN u64 task_word(u64 index, u32 sq, u32 rem, bool over) {
    return index | ((u64)sq << kSqShift) | ((u64)rem << kRemShift) | ((u64)over << kOverShift);
}
OTHC_FN u64 task_index(u64 w) { return w & kIndexMask; }
OTHC_FN u32 task_sq(u64 w) { return (u32)(w >> kSqShift) & 127u; }
OTHC_FN u32 task_rem(u64 w) { return (u32)(w >> kRemShift) & 15u; }
OTHC_FN bool task_over(u64 w) { return (w >> kOverShift) & 1u; }
// a task that is worth one path as it stands
OTHC_FN bool task_final(u64 w) { return task_over(w) || task_rem(w) == 0; }

struct Lane {
    u64 P, O, M;
    u64 count;
    u32 flags;
    int rem;    // plies left of the current frame
    int depth;  // of the current frame; < 0: no task
    u32 nodes;
    u32 status;  // set when the task ends (depth < 0 again)
};

// a task for the machine: mover's discs P, opponent's O (disjoint), 1 <= rem <=
// kMaxDepth plies left (task_final() tasks are worth 1 and need no machine)
OTHC_FN void start(Lane& L, u64 P, u64 O, int rem) {
    L.P = P;
    L.O = O;
    L.M = 0;
    L.count = 0;
    L.flags = kRootNew;
    L.rem = rem;
    L.depth = 0;
    L.nodes = 0;
    L.status = kCounted;
}

OTHC_FN void stop_at_limit(Lane& L) {
    L.depth = -1;
    L.count = 0;
    L.status = kLimit;
}

// POP: the current frame is done (M == 0, no flag: checked)
template <class S>
OTHC_FN void pop(Lane& L, S& stk) {
    if (L.depth == 0) {
        L.depth = -1;
        return;
    }
    L.depth--;
    L.rem++;
    stk.load(L.depth, L.P, L.O, L.M);
}

constexpr int kPopsPerStep = 2;  // as solve_core.hpp's

// one step of the lane's task; requires L.depth >= 0
template <class R, class S>
OTHC_FN void advance(Lane& L, S& stk, u32 limit) {
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int k = 0; k < kPopsPerStep; k++)
        if (L.depth >= 0 && L.M == 0 && L.flags == 0) pop(L, stk);
    if (L.depth < 0) return;
    u64 X, Y;  // the position to analyse: X to move
    int r = L.rem - 1;
    const bool mv = L.M != 0;
    if (mv) {
        const u32 sq = R::lowest(L.M);
        L.M &= L.M - 1;
        const u64 f = R::flips(sq, L.P, L.O);
        X = L.O & ~f;
        Y = L.P | f | (1ull << sq);
    } else if (L.flags & kRootNew) {
        X = L.P;
        Y = L.O;
        r = L.rem;
    } else if (L.flags & kFresh) {
        X = L.O;
        Y = L.P;
    } else {
        return;  // a third finished frame in a row: the next step pops it
    }
    if (L.nodes >= limit) return stop_at_limit(L);
    L.nodes++;
    const u64 cm = R::moves(X, Y);
    const bool root = (L.flags & kRootNew) != 0, check = !mv && !root;
    if (r <= 1) {  // the last ply in bulk (r == 0 never gets here: the root has r >= 1, a frame rem >= 2)
        L.count += cm ? (u64)R::count(cm) : 1ull;
        L.flags = 0;
        return;
    }
    if (cm == 0 && check) {  // neither side can move
        L.count += 1;
        L.flags = 0;
        return;
    }
    if (!root) {
        // (a task has at most kMaxDepth plies, so depth <= kFrames - 1 here;
        // the check keeps a defect out of the neighbours' frames)
        if (L.depth >= kFrames) return stop_at_limit(L);
        stk.store(L.depth, L.P, L.O, L.M);  // (a passing frame is stored too, with no move left)
        L.depth++;
    }
    L.P = X;
    L.O = Y;
    L.M = cm;
    L.rem = r;
    L.flags = cm ? 0u : kFresh;
}

}  // namespace othc
