// device_common.hpp — what the search files (solve.hip, search.hip, play.hip,
// tree.hip, solve_tree.hip) give their state machines on the device, and the
// host-side plumbing of their launches, stated once.
//   * DeviceRules: the rules parameter R of the cores, bitboard.hpp's moves()
//     and flips_carry(), the ones the step kernel plays by;
//   * DeviceAtomics: the atomics parameter A of the split trees' state words;
//   * LdsStack9 / LdsStack7: the stack parameter S, frames in LDS indexed
//     [depth][field][lane] in 32-bit words, so a wave's access is one word per
//     bank whatever depth each lane is at.  9 words: search_core.hpp's frame,
//     7: solve_core.hpp's;
//   * kRefillMin and take(): the device side of the work word, a wave's refill
//     of its idle lanes;
//   * status_of(), env_int(), ResidentBlocks, and the grid sizing of every
//     launch: launch_grid(), grid_answer().
// Everything device-side is force-inlined: no kernel gets a symbol from here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>

#include "../../include/othello.h"
#include "bitboard.hpp"

namespace othd {

typedef uint64_t u64;
typedef uint32_t u32;

// idle lanes that make a wave refill from the work word.  Measured with the
// solver (solve.hip's header); the other kernels take it over.
constexpr int kRefillMin = 8;

// THE WORK WORD, device side.  Every persistent kernel's items are handed out
// by one 64-bit word of the caller's:
//   * the word is 0 at launch;
//   * a wave whose idle lanes (`wantm`, `cnt` of them) refill makes one atomic
//     add of cnt by lane 0 and gives its wanting lanes base, base + 1, ... in
//     lane order; a lane whose index is not below the launch's items has made
//     its failing request and asks no more;
//   * every lane of the grid makes exactly one failing request, so the
//     launch's requests add up to `total` = items + lanes of the grid, and the
//     add that completes the sum resets the word: it is 0 again when the
//     launch ends, whatever the order the waves arrived in.
// take() is that turn, straight-line: the ballots, the refill predicate and the
// loop's break stay with the caller (moved in here they change the kernels'
// code).  Every lane of the wave calls it; the value is the
// lane's index where the lane is in wantm, and nothing elsewhere.
__device__ __forceinline__ u64 take(unsigned long long* work, u64 total, u64 wantm, u64 cnt, u32 lane) {
    u64 base = 0;
    if (lane == 0) {
        base = atomicAdd(work, cnt);
        if (base + cnt == total) atomicExch(work, 0ull);  // every request is made: reset
    }
    base = __shfl(base, 0);
    return base + (u64)__popcll(wantm & ((1ull << lane) - 1ull));
}

struct DeviceRules {
    static __device__ __forceinline__ u64 moves(u64 P, u64 O) { return oth::moves(P, O); }
    static __device__ __forceinline__ u64 flips(u32 sq, u64 P, u64 O) { return oth::flips_carry(sq, P, O); }
    static __device__ __forceinline__ u32 lowest(u64 m) { return (u32)__builtin_ctzll(m); }
    static __device__ __forceinline__ int count(u64 x) { return __popcll(x); }
    // int8 weight x count <= 64: exact in 24 bits, a full-rate multiply
    static __device__ __forceinline__ int mul(int w, int c) { return __mul24(w, c); }
};

struct DeviceAtomics {
    static __device__ __forceinline__ u64 load(u64* p) {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ bool cas(u64* p, u64& expected, u64 desired) {
        return __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
    }
    // an exchange whose return the lane waits for: the word is in place before
    // the lane's next atomic is issued
    static __device__ __forceinline__ void store(u64* p, u64 v) {
        const u64 old = __hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("" ::"v"(old) : "memory");
    }
};

// the search's frames in a block of kBlock lanes; `base` already points at the
// lane's column
template <int kBlock>
struct LdsStack9 {
    static constexpr int kFields = 9;
    u32* base;
    __device__ __forceinline__ u32* at(int depth) const { return base + depth * (kFields * kBlock); }
    __device__ __forceinline__ void store(int depth, u64 P, u64 O, u64 M, int alpha, int beta, u32 w) {
        u32* f = at(depth);
        f[0 * kBlock] = (u32)P;
        f[1 * kBlock] = (u32)(P >> 32);
        f[2 * kBlock] = (u32)O;
        f[3 * kBlock] = (u32)(O >> 32);
        f[4 * kBlock] = (u32)M;
        f[5 * kBlock] = (u32)(M >> 32);
        f[6 * kBlock] = (u32)alpha;
        f[7 * kBlock] = (u32)beta;
        f[8 * kBlock] = w;
    }
    __device__ __forceinline__ void load(int depth, u64& P, u64& O, u64& M, int& alpha, int& beta, u32& w) const {
        const u32* f = at(depth);
        P = (u64)f[0 * kBlock] | ((u64)f[1 * kBlock] << 32);
        O = (u64)f[2 * kBlock] | ((u64)f[3 * kBlock] << 32);
        M = (u64)f[4 * kBlock] | ((u64)f[5 * kBlock] << 32);
        alpha = (int)f[6 * kBlock];
        beta = (int)f[7 * kBlock];
        w = f[8 * kBlock];
    }
};

// the solver's frames: the window and the flags share the seventh word
template <int kBlock>
struct LdsStack7 {
    static constexpr int kFields = 7;
    u32* base;
    __device__ __forceinline__ u32* at(int depth) const { return base + depth * (kFields * kBlock); }
    __device__ __forceinline__ void store(int depth, u64 P, u64 O, u64 M, u32 w) {
        u32* f = at(depth);
        f[0 * kBlock] = (u32)P;
        f[1 * kBlock] = (u32)(P >> 32);
        f[2 * kBlock] = (u32)O;
        f[3 * kBlock] = (u32)(O >> 32);
        f[4 * kBlock] = (u32)M;
        f[5 * kBlock] = (u32)(M >> 32);
        f[6 * kBlock] = w;
    }
    __device__ __forceinline__ void load(int depth, u64& P, u64& O, u64& M, u32& w) const {
        const u32* f = at(depth);
        P = (u64)f[0 * kBlock] | ((u64)f[1 * kBlock] << 32);
        O = (u64)f[2 * kBlock] | ((u64)f[3 * kBlock] << 32);
        M = (u64)f[4 * kBlock] | ((u64)f[5 * kBlock] << 32);
        w = f[6 * kBlock];
    }
};

inline int status_of(hipError_t e) { return e == hipSuccess ? OTH_OK : -(int)e; }

inline int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

// blocks of one kernel a device holds at once, resolved on first use.  One
// object (static storage: zeroes) per kernel.
constexpr int kMaxDevices = 64;
struct ResidentBlocks {
    std::atomic<int> cached[kMaxDevices];
    // < 0: the current device is out of range
    int get(const void* kernel, int block) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (dev < 0 || dev >= kMaxDevices) return -1;
        int r = cached[dev].load(std::memory_order_acquire);
        if (r > 0) return r;
        int cus = 256, per_cu = 0;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0);
        (void)hipGetLastError();
        r = std::max(cus, 1) * (per_cu > 0 ? per_cu : 4);
        cached[dev].store(r, std::memory_order_release);  // (racing first calls compute the same value)
        return r;
    }
};

// blocks to launch for `items` work items in blocks of `block` lanes: no more
// than the kernel's resident blocks, than the environment variable `env` says
// (the tools' A/B) or than the items need.  at_least_one: an empty launch still
// runs one block (the split files).  <= 0: the current device is out of range.
inline int launch_grid(ResidentBlocks& cache, const void* kernel, int block, int64_t items, const char* env,
                       bool at_least_one = false) {
    const int resident = cache.get(kernel, block);
    if (resident <= 0) return -1;
    const int cap = std::min(std::max(env_int(env, resident), 1), resident);
    const int64_t need = (items + block - 1) / block;
    return (int)std::min<int64_t>(at_least_one ? std::max<int64_t>(need, 1) : need, (int64_t)cap);
}

// what a *_grid export answers for n items: OTH_EINVAL below 0, 0 for none
// (nothing asks the device), else grid(), or an error where that found none
template <class Grid>
inline int grid_answer(int64_t n, Grid grid) {
    if (n < 0) return OTH_EINVAL;
    if (n == 0) return 0;
    const int g = grid();
    return g > 0 ? g : status_of(hipErrorInvalidDevice);
}

}  // namespace othd
