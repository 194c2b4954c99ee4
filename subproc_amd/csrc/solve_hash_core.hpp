// solve_hash_core.hpp — the split solver's TRANSPOSITION TABLE: the entry, probe
// and store, and the hashed twins of solve_core.hpp's advance() and
// solve_order_core.hpp's advance_ordered().  Written once for the device
// (solve_tree.hip's hashed task kernels) and the host
// (tools/diag/solve_hash_host.cpp).  DESIGN.md §19 has the argument.
//
// AN ENTRY IS A PROOF.  32 bytes, four 64-bit words:
//   P, O    the position: the mover's discs and the opponent's, in full
//   bounds  byte 0 lower, byte 1 upper (int8 each): lower <= V(P to move) <= upper
//   seq     the slot's sequence word: even = at rest, odd = a writer is inside
// V is the exact solver's value, a fact about the position alone, so an entry
// is true in any later call, under either move order.  All zero is an empty
// slot (no probed position has P = O = 0).  One slot per position (the high
// `bits` bits of a mix of P and O), always replaced; when the slot holds the
// same position, the bounds are intersected.
//
// THE SLOT IS A SEQLOCK IN WHICH NOBODY WAITS.  The atomics policy A names the
// accesses; every word of the table is touched through it only.
//   writer  s = load(seq); odd: DROP.  claim(seq, s, s + 1) fails: DROP.  Then
//           the three data words, then publish(seq, s + 2).
//   reader  s1 = load(seq), the data words, s2 = load(seq): a hit needs s1 even,
//           s2 == s1 and both boards equal to its own, word for word; anything
//           else is a miss.  A miss needs no ordering, so a first unordered
//           look sorts the misses out before the ordered one.
// What A must give (DESIGN.md §19 derives the guarantee from exactly this):
//   claim    a compare-and-swap that is an ACQUIRE, and whose success comes
//            before the writer's data stores for every observer (a release
//            fence behind it, or data stores that are releases themselves);
//   publish  a RELEASE store;
//   seq_load / read_fence / data_load
//            the reader's first look at seq is an ACQUIRE before its data
//            loads, and its data loads come before its second look at seq (an
//            acquire fence between them, or data loads that are acquires).
// The device's policy spells these with agent-scope fences around relaxed
// atomics, the host's thread policy with orderings on the accesses themselves
// (ThreadSanitizer does not model a stand-alone fence).
//
// THE SEARCH STAYS FAIL-HARD.  A child that is about to be pushed and has at
// least `min_empties` empty squares is probed.  With (a, b) the window the
// child would get, the probe answers for it in three cases, with the very
// value the child's search would hand up, clamp(V, a, b):
//   upper <= a: a;   lower >= b: b;   lower == upper: clamp(lower, a, b).
// Nothing else is done with an entry: no window is narrowed.  So no return
// changes, every window further on is what it was, and in a fixed task order the
// hashed search's nodes are a subset of the unhashed search's.
// A frame that finishes (and only then: a task stopped at the node limit
// stores nothing) stores what its return proves; kRaised, one more flag bit in
// the packed word, remembers whether a score ever raised its alpha:
//   alpha >= beta: V >= beta;   never raised: V <= alpha;   else V == alpha.
// A frame entered by a pass stores under the board it was pushed with (the
// passer to move), the value negated.  A task's own depth-0 frame is a node of
// the expanded tree: it is never probed, and it stores when it finishes.
#pragma once
#include <stdint.h>

#include "solve_order_core.hpp"

namespace othh {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr int kMinBits = 4;        // OTHH_MIN_BITS: 16 entries
constexpr int kMaxBits = 26;       // OTHH_MAX_BITS: 2 GiB
constexpr int kMinGate = 1;        // OTHH_MIN_EMPTIES_LO
constexpr int kMaxGate = 12;       // OTHH_MIN_EMPTIES_HI
constexpr int kDefaultGate = 8;    // OTHH_DEFAULT_MIN_EMPTIES
constexpr int kEntryBytes = 32;    // OTHH_ENTRY_BYTES

constexpr u32 kRaised = 8;         // beside oths::kFresh / kPassed / kRootNew: a score raised the frame's alpha
constexpr int kNoBound = 65;       // the solver's own infinity

struct Entry {
    u64 P, O, bounds, seq;
};
static_assert(sizeof(Entry) == kEntryBytes, "entry layout");

struct Table {
    Entry* e;
    int shift;        // 64 - bits
    int min_empties;  // frames with fewer empties neither probe nor store
};

OTHS_FN u64 pack_bounds(int lo, int hi) { return (u64)(u32)(lo & 0xFF) | ((u64)(u32)(hi & 0xFF) << 8); }
OTHS_FN int lower_of(u64 w) { return (int)(int8_t)(w & 0xFF); }
OTHS_FN int upper_of(u64 w) { return (int)(int8_t)((w >> 8) & 0xFF); }

OTHS_FN u64 slot_of(const Table& t, u64 P, u64 O) {
    u64 h = P * 0x9E3779B97F4A7C15ull;
    h ^= h >> 32;
    h += O * 0xC2B2AE3D27D4EB4Full;
    h ^= h >> 29;
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    h *= 0x9E3779B97F4A7C15ull;
    return h >> t.shift;
}

// the bounds the table proves for (P to move, O); false: nothing (lo, hi untouched)
template <class A>
OTHS_FN bool probe(const Table& t, u64 P, u64 O, int& lo, int& hi) {
    Entry* e = t.e + slot_of(t, P, O);
    // the first look: a miss needs no ordering
    const u64 s1 = A::seq_load(&e->seq);
    u64 p = A::data_load(&e->P), o = A::data_load(&e->O);
    if ((s1 & 1) || p != P || o != O) return false;
    // the ordered look: s1 before the data, the data before s2
    A::read_fence();
    p = A::data_load(&e->P);
    o = A::data_load(&e->O);
    const u64 b = A::data_load(&e->bounds);
    A::read_fence();
    const u64 s2 = A::load(&e->seq);
    if (s2 != s1 || p != P || o != O) return false;
    lo = lower_of(b);
    hi = upper_of(b);
    return true;
}

// lower <= V(P to move, O) <= upper is proved: put it into the position's slot
template <class A>
OTHS_FN void store(const Table& t, u64 P, u64 O, int lo, int hi) {
    Entry* e = t.e + slot_of(t, P, O);
    const u64 s = A::load(&e->seq);
    if (s & 1) return;                          // a writer is inside: drop
    // an unordered look, which decides only what may always be decided freely:
    // to drop a store that seems to add nothing, and whether to look again
    const bool same = A::load(&e->P) == P && A::load(&e->O) == O;
    if (same) {
        const u64 b = A::load(&e->bounds);
        if (lower_of(b) >= lo && upper_of(b) <= hi) return;
    }
    if (!A::claim(&e->seq, s, s + 1)) return;   // another writer was faster: drop
    // the slot is this writer's: every earlier writer's words are in place
    if (same && A::data_load(&e->P) == P && A::data_load(&e->O) == O) {
        const u64 b = A::data_load(&e->bounds);
        const int l = lower_of(b), h = upper_of(b);
        if (l > lo) lo = l;
        if (h < hi) hi = h;
    }
    A::data_store(&e->P, P);
    A::data_store(&e->O, O);
    A::data_store(&e->bounds, pack_bounds(lo, hi));
    A::publish(&e->seq, s + 2);
}

OTHS_FN void apply_score_hashed(oths::Lane& L, int score) {
    if (score > L.alpha) L.flags |= kRaised;
    oths::apply_score(L, score);
}

// what the finished current frame proves goes into the table
template <class R, class A>
OTHS_FN void store_frame(const oths::Lane& L, const Table& t) {
    if (64 - R::count(L.P | L.O) < t.min_empties) return;
    int lo = -kNoBound, hi = kNoBound;
    if (L.alpha >= L.beta)
        lo = L.beta;
    else if (!(L.flags & kRaised))
        hi = L.alpha;
    else
        lo = hi = L.alpha;
    if (L.flags & oths::kPassed)  // the frame was pushed, and probed, as the passer's
        store<A>(t, L.O, L.P, -hi, -lo);
    else
        store<A>(t, L.P, L.O, lo, hi);
}

// oths::pop() with the store in front and the flag kept
template <class R, class A, class S>
OTHS_FN void pop_hashed(oths::Lane& L, S& stk, const Table& t) {
    store_frame<R, A>(L, t);
    const int score = (L.flags & oths::kPassed) ? L.alpha : -L.alpha;  // for the parent's mover
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
    apply_score_hashed(L, score);
}

template <class R, class A, class S>
OTHS_FN void pops_hashed(oths::Lane& L, S& stk, const Table& t) {
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int r = 0; r < oths::kPopsPerStep; r++)
        if (L.depth >= 0 && L.M == 0 && !(L.flags & (oths::kFresh | oths::kRootNew))) pop_hashed<R, A>(L, stk, t);
}

// the step's second half for a placed move: the child (X to move, Y) with the
// moves cm.  Board full and the table's three cases end it here; everything
// else is oths::settle_child()'s.
template <class R, class A, class S>
OTHS_FN void settle_hashed(oths::Lane& L, S& stk, const Table& t, u32 limit, bool mv, u64 X, u64 Y, u64 cm) {
    if (mv) {
        if (~(X | Y) == 0) return apply_score_hashed(L, R::count(Y) - R::count(X));
        if (64 - R::count(X | Y) >= t.min_empties) {
            int lo = -kNoBound, hi = kNoBound;
            if (probe<A>(t, X, Y, lo, hi)) {
                const int a = -L.beta, b = -L.alpha;  // the child's window
                if (hi <= a) return apply_score_hashed(L, -a);
                if (lo >= b) return apply_score_hashed(L, -b);
                if (lo == hi) return apply_score_hashed(L, -lo);
            }
        }
    }
    oths::settle_child<R>(L, stk, limit, mv, X, Y, cm);
}

// advance() with the table: one step of the lane's search; requires L.depth >= 0
template <class R, class A, class S>
OTHS_FN void advance_hashed(oths::Lane& L, S& stk, const Table& t, u32 limit) {
    pops_hashed<R, A>(L, stk, t);
    if (L.depth < 0) return;
    u64 X, Y;  // the position to analyse: X to move
    const bool mv = L.M != 0;
    if (mv) {
        if (L.nodes >= limit) return oths::stop_at_limit(L);
        const u32 sq = R::lowest(L.M);
        const u64 bit = 1ull << sq;
        L.M &= L.M - 1;
        const u64 f = R::flips(sq, L.P, L.O);
        X = L.O & ~f;
        Y = L.P | f | bit;
        if (L.depth == 0) L.root_mv = sq;
        L.nodes++;
    } else if (L.flags & oths::kRootNew) {
        X = L.P;
        Y = L.O;
    } else if (L.flags & oths::kFresh) {
        X = L.O;
        Y = L.P;
    } else {
        return;  // a third finished frame in a row: the next step pops it
    }
    const u64 cm = R::moves(X, Y);
    settle_hashed<R, A>(L, stk, t, limit, mv, X, Y, cm);
}

// advance_ordered() with the table; Q reset when the task started
template <class R, class A, class S>
OTHS_FN void advance_ordered_hashed(oths::Lane& L, othm::Order& Q, S& stk, const Table& t, u32 limit) {
    pops_hashed<R, A>(L, stk, t);
    if (L.depth < 0) return;
    u64 X, Y;  // the position to analyse: X to move
    const bool mv = L.M != 0;
    bool scoring = false;
    u32 sq = 0;
    if (mv) {
        if (L.nodes >= limit) return oths::stop_at_limit(L);
        othm::order_begin(Q, L.M, [&] { return 64 - R::count(L.P | L.O) >= oths::kMobilityEmpties; });
        scoring = Q.cand != 0;
        sq = scoring ? othm::order_candidate<R>(Q) : othm::order_choice<R>(Q, L.M);
        const u64 bit = 1ull << sq;
        const u64 f = R::flips(sq, L.P, L.O);
        X = L.O & ~f;
        Y = L.P | f | bit;
        L.nodes++;
        if (!scoring) {
            Q.pick = othm::kPickNone;
            L.M &= ~bit;
            if (L.depth == 0) L.root_mv = sq;
        }
    } else if (L.flags & oths::kRootNew) {
        X = L.P;
        Y = L.O;
    } else if (L.flags & oths::kFresh) {
        X = L.O;
        Y = L.P;
    } else {
        return;  // a third finished frame in a row: the next step pops it
    }
    const u64 cm = R::moves(X, Y);
    if (scoring) {
        const u32 corner = (othm::kRegion0 >> sq) & 1u ? 0u : (u32)othm::kCornerBonus;
        return othm::order_keep(Q, (((u32)R::count(cm) + corner) << 6) | sq);
    }
    settle_hashed<R, A>(L, stk, t, limit, mv, X, Y, cm);
}

}  // namespace othh
