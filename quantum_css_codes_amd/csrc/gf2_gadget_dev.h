// The tally rules of the two post-selected gadgets on one lane's outcome words, as __forceinline__ device functions: the chain of
// ec_kernel (gf2_ec.hip) and the step walk of ft_kernel (gf2_ft.hip), which gadget_enumerate_kernel (gf2_gadget_enumerate.hip) and
// gadget_strata_kernel (gf2_gadget_strata.hip) call.  The two samplers keep their own text of the same rule: calling these functions from them moved their register counts
// (DESIGN.md "Exact strata of the cycle", "Kernel"), and tests/test_gpu_gadget_enumerate.py holds the two texts together through
// the host statement.  Both rules are fully unrolled over constant word indices under uniform guards, so out[] never takes a
// run-time index (it would go to scratch).  Args: a kernel's argument block with mask[2], tab[2], flips[2] and rounds (the cycle)
// or nsteps, measure_mask, first_measure (the measurement).
#pragma once

#include "gf2_circuit_dev.h"

// The OR of the cycle's flag words (words rounds + 1 .. LDR - 1): not zero -- a verification fired, the attempt is rejected.
template <int LDR, class Args>
__device__ __forceinline__ u64 ec_flag_or(const Args& a, const u64 (&out)[LDR]) {
    u64 flags = 0;
#pragma unroll
    for (int w = 2; w < LDR; ++w) flags |= w > a.rounds ? out[w] : 0ull;           // (word 1 is a round's: rounds >= 1)
    return flags;
}

// The chain of an accepted sample of the cycle: round t's key decoded relative to the syndrome K of what earlier rounds recorded,
// then the final frame judged against the record.  unmatched[side] (two counters, constant index) is added to.
template <int LDR, class Args>
__device__ __forceinline__ void ec_chain(const Args& a, const u64 (&out)[LDR], bool (&flip)[2], bool (&miss)[2], unsigned int* unmatched) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        u64 K = 0;                                                                 // syndrome of the errors recorded so far
        unsigned int P = 0;                                                        // ... and their operator parity
#pragma unroll
        for (int t = 1; t <= GF2_EC_MAX_ROUNDS; ++t) {
            if (t <= LDR - 2 && t <= a.rounds) {
                const u64 s = ((out[t < LDR ? t : 0] >> (32 * c)) & a.mask[c]) ^ K;
                const u64 slot = hash_find<1>(a.tab[c], 0ull, s);
                if (slot == ~0ull) {
                    unmatched[c] += 1;                                            // css_code.py:655-657: no match, nothing recorded
                } else {
                    K ^= s;
                    P ^= a.flips[c][a.tab[c].val[slot]] & 1u;
                }
            }
        }
        const u64 s = ((out[0] >> (32 * c)) & a.mask[c]) ^ K;
        const u64 slot = hash_find<1>(a.tab[c], 0ull, s);
        miss[c] = slot == ~0ull;
        unsigned int f = (unsigned int)((out[0] >> (32 * c + 31)) & 1ull) ^ P;
        if (!miss[c]) f ^= a.flips[c][a.tab[c].val[slot]] & 1u;
        flip[c] = f != 0;
    }
}

// The OR of the measurement's flag words (words nsteps .. LDR - 1).
template <int LDR, class Args>
__device__ __forceinline__ u64 ft_flag_or(const Args& a, const u64 (&out)[LDR]) {
    u64 flags = 0;
#pragma unroll
    for (int w = 1; w < LDR; ++w) flags |= w >= a.nsteps ? out[w] : 0ull;          // (word 0 is a step's: nsteps >= 1)
    return flags;
}

// The step walk of an accepted sample of the measurement: one record of known errors per side (syndrome K, operator parity P) run
// through the steps in order; a trial's bit is read against everything recorded up to and including its own key.
template <int LDR, class Args>
__device__ __forceinline__ void ft_walk(const Args& a, const u64 (&out)[LDR], unsigned int& wrong_trials, unsigned int& first_wrong,
                                        unsigned int* unmatched) {
    u64 K[2] = {0, 0};                                                             // syndrome of the errors recorded so far, per side
    unsigned int P[2] = {0, 0};                                                    // ... and their operator parity
#pragma unroll
    for (int s = 0; s < LDR - 1; ++s) {
        if (s < a.nsteps) {
            const bool measure = (a.measure_mask >> s) & 1u;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (c == 0 || !measure) {                                          // a measurement corrects data.x_errors only
                    const u64 v = ((out[s] >> (32 * c)) & a.mask[c]) ^ K[c];
                    const u64 slot = hash_find<1>(a.tab[c], 0ull, v);
                    if (slot == ~0ull) {
                        unmatched[c] += 1;                                        // css_code.py:655-657: no match, nothing recorded
                    } else {
                        K[c] ^= v;
                        P[c] ^= a.flips[c][a.tab[c].val[slot]] & 1u;
                    }
                }
            }
            if (measure) {
                const unsigned int bad = (unsigned int)((out[s] >> 31) & 1ull) ^ P[0];
                wrong_trials += bad;
                if (s == a.first_measure) first_wrong = bad;
            }
        }
    }
}
