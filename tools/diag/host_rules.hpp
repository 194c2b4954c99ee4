// host_rules.hpp — what every host build of the cores (tools/diag/*_host.cpp;
// tools/diag/README.md lists them) gives the cores in place of the device's
// parameters: a plain C++ statement of the rules (R), plain loads and stores for
// the atomics (A) and arrays for the frames (S).  The files the programs read
// are host_io.hpp's.
#pragma once
#include <stdint.h>

// the rules, stated over whole boards one direction at a time (the 16-empties
// roots need a host build that makes some ten million nodes a second)
struct HostRules {
    typedef uint64_t u64;
    typedef uint32_t u32;
    // a board moved one square in direction d: east, south-west, south, south-east, then their opposites
    static u64 step(u64 x, int d) {
        switch (d) {
            case 0: return (x << 1) & 0xFEFEFEFEFEFEFEFEull;
            case 1: return (x << 7) & 0x7F7F7F7F7F7F7F7Full;
            case 2: return x << 8;
            case 3: return (x << 9) & 0xFEFEFEFEFEFEFEFEull;
            case 4: return (x >> 1) & 0x7F7F7F7F7F7F7F7Full;
            case 5: return (x >> 7) & 0xFEFEFEFEFEFEFEFEull;
            case 6: return x >> 8;
            default: return (x >> 9) & 0x7F7F7F7F7F7F7F7Full;
        }
    }
    static int count(u64 x) { return __builtin_popcountll(x); }
    static u32 lowest(u64 m) { return (u32)__builtin_ctzll(m); }
    static int mul(int w, int c) { return w * c; }
    // the opponent discs the move on empty square sq turns over
    static u64 flips(u32 sq, u64 P, u64 O) {
        u64 all = 0;
        for (int d = 0; d < 8; d++) {
            u64 run = 0, x = step(1ull << sq, d);
            while (x & O) {
                run |= x;
                x = step(x, d);
            }
            if (x & P) all |= run;
        }
        return all;
    }
    // the empty squares from which a run of O ends on a disc of P
    static u64 moves(u64 P, u64 O) {
        u64 m = 0;
        for (int d = 0; d < 8; d++) {
            u64 run = step(P, d) & O;
            for (int k = 0; k < 5; k++) run |= step(run, d) & O;
            m |= step(run, d);
        }
        return m & ~(P | O);
    }
};

// one thread touches a position's tree at a time
struct HostAtomics {
    typedef uint64_t u64;
    static u64 load(u64* p) { return *p; }
    static bool cas(u64* p, u64& expected, u64 desired) {
        if (*p != expected) {
            expected = *p;
            return false;
        }
        *p = desired;
        return true;
    }
    static void store(u64* p, u64 v) { *p = v; }
};

// search_core.hpp's frames (kFrames = othm::kFrames)
template <int kFrames>
struct HostStack9 {
    typedef uint64_t u64;
    typedef uint32_t u32;
    u64 P[kFrames], O[kFrames], M[kFrames];
    int a[kFrames], b[kFrames];
    u32 w[kFrames];
    void store(int d, u64 p, u64 o, u64 m, int al, int be, u32 ww) {
        P[d] = p, O[d] = o, M[d] = m, a[d] = al, b[d] = be, w[d] = ww;
    }
    void load(int d, u64& p, u64& o, u64& m, int& al, int& be, u32& ww) const {
        p = P[d], o = O[d], m = M[d], al = a[d], be = b[d], ww = w[d];
    }
};

// solve_core.hpp's frames (kFrames = oths::kFrames)
template <int kFrames>
struct HostStack7 {
    typedef uint64_t u64;
    typedef uint32_t u32;
    u64 P[kFrames], O[kFrames], M[kFrames];
    u32 w[kFrames];
    void store(int d, u64 p, u64 o, u64 m, u32 ww) { P[d] = p, O[d] = o, M[d] = m, w[d] = ww; }
    void load(int d, u64& p, u64& o, u64& m, u32& ww) const { p = P[d], o = O[d], m = M[d], ww = w[d]; }
};
