// The wait draw of one attempt of a retried region (DESIGN.md section 5d "Repeat-until-success with waiting faults", include/gf2hip.h):
// what the data block picks up while it waits through attempt `att`, passed or not.  Device code of gf2_retry_gate_wait.hip;
// gf2_retry_wait.hip keeps its own copy of these lines (its generated code is left as it was).
#pragma once

#include "gf2_sampler.h"

// One error_count under the wait key of (region, attempt) -- kw = segment_draw(ks, GF2_RETRY_WAIT_SLOT_BASE + g) is the caller's --
// usually K = 0; the picks by Floyd's rule against the lane's taken map `mine`, free between the region's own draws; the kinds
// error_draw's with q's thresholds.  rows: the region's W wait rows, four words each (X local, X tail, Z local, Z tail), in LDS when
// ROWS_LDS holds and in device memory otherwise.  A position is below W, so its row is one of the region's.  XORs into (wl, wt), which
// the caller never clears between attempts, and returns K.
template <bool ROWS_LDS>
__device__ __forceinline__ int retry_wait_draw(u64 kw, int att, int W, const u64* cdf, u64 w_1, u64 w_2, const u64* rows, unsigned int* mine, u64& wl,
                                               u64& wt) {
    const u64 d = segment_draw(mix64(kw + GF2_GOLDEN * (u64)(att + 1)), 0ull);
    const int K = error_count(d, W, cdf);
    if (K > 1)
        for (int w = 0; w < (W + 31) >> 5; ++w) mine[w] = 0;
    for (int k = 0; k < K; ++k) {
        unsigned int pick, kind;
        error_draw(d, k, K, W, w_1, w_2, &pick, &kind);
        unsigned int pos = pick;
        if (K > 1) {                                                           // Floyd's rule: a candidate already taken -> j
            if ((mine[pick >> 5] >> (pick & 31u)) & 1u) pos = (unsigned int)(W - K + k);
            mine[pos >> 5] |= 1u << (pos & 31u);
        }
        const u64* e = rows + (size_t)pos * 4;
        const u64 xl = e[0], xt = e[1], zl = e[2], zt = e[3];
        if (kind & 1u) wl ^= xl, wt ^= xt;
        if (kind & 2u) wl ^= zl, wt ^= zt;
    }
    return K;
}
