// The walk of an enumerated rank range (DESIGN.md "Exact strata"), shared by enumerate_kernel (gf2_enumerate.hip),
// gadget_enumerate_kernel (gf2_gadget_enumerate.hip), gadget_list_kernel (gf2_gadget_list.hip) and, for its unranking and its launch
// shape, gate_enumerate_kernel (gf2_gate_enumerate.hip): how a launch is cut into runs and workgroups (host side), exact binomials,
// unranking in the combinatorial number system, the colexicographic successor and one step of the reflected ternary Gray code over
// the digit order X, Y, Z.  Every device function is __forceinline__, works on eight picks held in VGPRs and indexes them with
// constants or with selects on a scalar only.
#pragma once

#include "gf2_circuit_dev.h"

#define ENUM_MAX_W GF2_ENUMERATE_MAX_WEIGHT
#define ENUM_LAUNCH_CONFIGS (1ll << 30)        // configurations per launch (DESIGN.md "Exact strata")
#define ENUM_MAX_RUN 32                        // ranks per lane and unranking
#define ENUM_MAX_BLOCKS 2048                   // 8 workgroups of 256 lanes on each of the 256 CUs

// The shape of a launch over `count` subsets: *run consecutive ranks per lane -- short runs until every lane of ENUM_MAX_BLOCKS
// workgroups has one, at most ENUM_MAX_RUN -- and the workgroups that cover the runs.
static void enum_launch_shape(int64_t count, int* run, unsigned* blocks) {
    const int64_t r = count / ((int64_t)ENUM_MAX_BLOCKS * CIRC_THREADS);
    *run = (int)(r < 1 ? 1 : r > ENUM_MAX_RUN ? ENUM_MAX_RUN : r);
    const int64_t b = gf2_cdiv(gf2_cdiv(count, *run), CIRC_THREADS);
    *blocks = (unsigned)(b > ENUM_MAX_BLOCKS ? ENUM_MAX_BLOCKS : b);
}

// C(s, K) for s < L, exact: c_i = C(s - K + i, i) -> c_{i+1} = c_i (s - K + 1 + i) / (i + 1), the division split so that no
// intermediate exceeds the result (below C(L, w) < 2^63).  The divisors are constants after unrolling.
template <int K>
__device__ __forceinline__ u64 enum_binom(u64 s) {
    if (s < (u64)K) return 0;
    u64 c = 1;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const u64 m = s - K + 1 + i, d = i + 1;
        c = (c / d) * m + ((c % d) * m) / d;
    }
    return c;
}

// Pick K - 1 of the subset of rank r: the largest s in [K - 1, hi) with C(s, K) <= r.  hi and r are updated for the pick below.
template <int K>
__device__ __forceinline__ unsigned int enum_unrank_pick(u64& r, unsigned int& hi) {
    unsigned int lo = K - 1;
    while (hi - lo > 1) {
        const unsigned int mid = lo + ((hi - lo) >> 1);
        if (enum_binom<K>(mid) <= r) lo = mid; else hi = mid;
    }
    r -= enum_binom<K>(lo);
    hi = lo;
    return lo;
}

// The w picks of the subset of rank r among `locations` (the picks from w up are 0).
__device__ __forceinline__ void enum_unrank(int w, u64 r, unsigned int locations, unsigned int (&pos)[ENUM_MAX_W]) {
    unsigned int hi = locations;
    pos[7] = w > 7 ? enum_unrank_pick<8>(r, hi) : 0u;
    pos[6] = w > 6 ? enum_unrank_pick<7>(r, hi) : 0u;
    pos[5] = w > 5 ? enum_unrank_pick<6>(r, hi) : 0u;
    pos[4] = w > 4 ? enum_unrank_pick<5>(r, hi) : 0u;
    pos[3] = w > 3 ? enum_unrank_pick<4>(r, hi) : 0u;
    pos[2] = w > 2 ? enum_unrank_pick<3>(r, hi) : 0u;
    pos[1] = w > 1 ? enum_unrank_pick<2>(r, hi) : 0u;
    pos[0] = w > 0 ? enum_unrank_pick<1>(r, hi) : 0u;
}

// Successor: the lowest pick that can move up does, the picks below it fall back to 0, 1, ...  (a live subset is not the last of
// all, so the pick that moves stays below L)
__device__ __forceinline__ void enum_successor(int w, unsigned int (&pos)[ENUM_MAX_W]) {
    bool done = false;
#pragma unroll
    for (int j = 0; j < ENUM_MAX_W; ++j) {
        if (j < w && !done) {
            const bool can = j == w - 1 || pos[j] + 1 < pos[j + 1 < ENUM_MAX_W ? j + 1 : j];
            pos[j] = can ? pos[j] + 1 : (unsigned int)j;
            done = can;
        }
    }
}

// Trip t > 0 of the Gray code: digit j moves, a = digit j of t (not 0), reflected when the digits above it make an odd number.
// Returns the pick whose kind changes; xy: X <-> Y (XOR its Z effect), else Y <-> Z (its X effect); the composition follows.
__device__ __forceinline__ unsigned int enum_gray_step(unsigned int t, const unsigned int (&pos)[ENUM_MAX_W], bool& xy, int& n_x, int& n_y) {
    unsigned int q3 = t;
    int j = 0;
    while (q3 % 3u == 0u) q3 /= 3u, ++j;
    const unsigned int digit = q3 % 3u, above = q3 / 3u;
    const unsigned int now = (above & 1u) ? 2u - digit : digit, was = (above & 1u) ? 3u - digit : digit - 1u;
    xy = (now < was ? now : was) == 0u;                                   // X <-> Y: the Z effect; Y <-> Z: the X effect
    n_x += (was == 0u) ? -1 : (now == 0u) ? 1 : 0;
    n_y += (now == 1u) ? 1 : -1;
    // (selects on the scalar j between the eight values, every pick read first: a pick read under its condition would become a
    // load at a selected address, and the picks would go to scratch)
    const unsigned int p0 = pos[0], p1 = pos[1], p2 = pos[2], p3 = pos[3], p4 = pos[4], p5 = pos[5], p6 = pos[6], p7 = pos[7];
    unsigned int p = p0;
    p = j == 1 ? p1 : p;
    p = j == 2 ? p2 : p;
    p = j == 3 ? p3 : p;
    p = j == 4 ? p4 : p;
    p = j == 5 ? p5 : p;
    p = j == 6 ? p6 : p;
    p = j == 7 ? p7 : p;
    return p;
}

// The outcome words of the all-X assignment of a subset.
template <int LDR>
__device__ __forceinline__ void enum_all_x(int w, const u64* eff, const unsigned int (&pos)[ENUM_MAX_W], u64 (&out)[LDR]) {
#pragma unroll
    for (int q = 0; q < LDR; ++q) out[q] = 0;
#pragma unroll
    for (int k = 0; k < ENUM_MAX_W; ++k) {
        if (k < w) {
            const u64* e = eff + (size_t)(2 * pos[k]) * LDR;
#pragma unroll
            for (int q = 0; q < LDR; ++q) out[q] ^= e[q];
        }
    }
}
