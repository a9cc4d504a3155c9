// The draw of one class of a retried region's sites under gate-level faults (DESIGN.md section 5d "Repeat-until-success under
// gate-level faults"): device code shared by gf2_retry_gate.hip and gf2_retry_gate_wait.hip.
#pragma once

#include "gf2_circuit_dev.h"

// The faults of one class of a region's sites under the attempt key `ka`, XOR-ed into (l, t, f): gf2_gate_mc.hip's gate_class_gather
// over the m sites from site_base on, with the region's own tables (cdf_last: its last segment's, cdf_full: a whole segment's).  A
// position is below nb, so its site is one of the region's, and the rows its mask names -- site[.] and, for a CNOT, the next -- lie
// inside the region (the site table is checked on the host).
template <bool CNOT>
__device__ __forceinline__ void retry_gate_class(int m, int site_base, const u64* cdf_last, const u64* cdf_full, const u64* eff, const int* site,
                                                 unsigned int* mine, u64 ka, u64& l, u64& t, u64& f) {
    const int nseg = (m + GF2_SEG_BITS - 1) / GF2_SEG_BITS;
    for (int s = 0; s < nseg; ++s) {
        const bool last = s == nseg - 1;
        const int nb = last ? m - s * GF2_SEG_BITS : GF2_SEG_BITS;
        const u64 d = segment_draw(ka, (u64)((CNOT ? GF2_GATE_MC_SLOT_CNOT : GF2_GATE_MC_SLOT_ONE) + s));
        const int K = error_count(d, nb, last ? cdf_last : cdf_full);
        if (K > 1)
            for (int w = 0; w < (nb + 31) >> 5; ++w) mine[w] = 0;
        for (int k = 0; k < K; ++k) {
            const u64 v = mix64(d + GF2_GOLDEN * (u64)(k + 1));
            const u64 hi = v >> 32, lo = v & 0xFFFFFFFFull;
            const unsigned int j = (unsigned int)(nb - K + k);
            const unsigned int pick = (unsigned int)((hi * (u64)(j + 1u)) >> 32);
            unsigned int pos = pick;
            if (K > 1) {                                                       // Floyd's rule: a candidate already taken -> j
                if ((mine[pick >> 5] >> (pick & 31u)) & 1u) pos = j;
                mine[pos >> 5] |= 1u << (pos & 31u);
            }
            const unsigned int kappa = 1u + (unsigned int)((lo * (CNOT ? 15ull : 3ull)) >> 32);
            const u64* e = eff + (size_t)site[site_base + s * GF2_SEG_BITS + (int)pos] * 6;
            if (kappa & 1u) l ^= e[0], t ^= e[1], f ^= e[2];
            if (kappa & 2u) l ^= e[3], t ^= e[4], f ^= e[5];
            if (CNOT) {                                                        // the target's two effects: the next row
                if (kappa & 4u) l ^= e[6], t ^= e[7], f ^= e[8];
                if (kappa & 8u) l ^= e[9], t ^= e[10], f ^= e[11];
            }
        }
    }
}
