// What the entry points of the two post-selected gadgets share -- gf2_ec.hip and gf2_ft.hip (the two samplers), gf2_gadget_strata.hip
// (the sampled strata), gf2_gadget_enumerate.hip (the exact strata), gf2_gate_enumerate.hip (the exact strata under gate-level
// faults) and gf2_gadget_list.hip (the malignant fault sets).
//
// Host side: the rule setup of an argument block (ec_rule_args, ft_rule_args: the argument rules of gf2_gadget_rule.h on a circuit)
// and the dispatch of a launch on the circuit's words per effect (gadget_for_ldr).
//
// Device side: the tally rules on one lane's outcome words, as __forceinline__ device functions -- the chain of ec_kernel
// (gf2_ec.hip) and the step walk of ft_kernel (gf2_ft.hip), which gadget_enumerate_kernel, gate_enumerate_kernel, gadget_list_kernel
// and gadget_strata_kernel call -- and the wavefront tally of the two counting kernels (gadget_enumerate_kernel,
// gate_enumerate_kernel).  The two samplers keep their own text of the same rule: calling these functions from them moved their register counts
// (DESIGN.md "Exact strata of the cycle", "Kernel"), and tests/test_gpu_gadget_enumerate.py holds the two texts together through
// the host statement.  Both rules are fully unrolled over constant word indices under uniform guards, so out[] never takes a
// run-time index (it would go to scratch).  Args: a kernel's argument block with mask[2], tab[2], flips[2] and rounds (the cycle)
// or nsteps, measure_mask, first_measure (the measurement).
#pragma once

#include <type_traits>

#include "gf2_circuit_dev.h"
#include "gf2_gadget_rule.h"

enum { RULE_EC = 0, RULE_FT = 1 };
#define FT_MIN_LDR 8                           // the device entry points of the measurement take 8 .. GF2_FT_MAX_LDR words per effect

// The rule fields of a cycle's argument block from checked arguments: the layout, then the circuit's effects against it.
template <class Args>
static int ec_rule_args(const char* who, const gf2_circuit* circuit, int64_t rounds, int64_t r1, int64_t r2, Args* a) {
    GadgetRule rule;
    GF2_TRY(ec_rule_layout(who, circuit->ldr, rounds, r1, r2, &rule));
    GF2_TRY(ec_rule_effects(who, (const uint64_t*)circuit->any, rounds, rule));
    a->rounds = (int)rounds;
    a->mask[0] = rule.mask[0];
    a->mask[1] = rule.mask[1];
    a->kwx = a->kwz = 1;
    return GF2_OK;
}

// ... and of a measurement's.
template <class Args>
static int ft_rule_args(const char* who, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1, int64_t r2, Args* a) {
    GadgetRule rule;
    GF2_TRY(ft_rule_layout(who, circuit->ldr, FT_MIN_LDR, nsteps, measure_mask, r1, r2, &rule));
    GF2_TRY(ft_rule_effects(who, (const uint64_t*)circuit->any, nsteps, measure_mask, rule));
    a->nsteps = (int)nsteps;
    a->trials = rule.trials;
    a->first_measure = rule.first_measure;
    a->measure_mask = (unsigned int)measure_mask;
    a->mask[0] = rule.mask[0];
    a->mask[1] = rule.mask[1];
    a->kwx = a->kwz = 1;
    return GF2_OK;
}

// f(std::integral_constant<int, L>) for the one L in [FIRST, LAST] that equals ldr ...
template <int FIRST, int LAST, class F>
static void ldr_dispatch(int64_t ldr, F& f) {
    if (ldr == FIRST)
        f(std::integral_constant<int, FIRST>{});
    else if constexpr (FIRST < LAST)
        ldr_dispatch<FIRST + 1, LAST>(ldr, f);
}

// ... over the words per effect a rule's kernels are instantiated for: 3 .. 8 (the cycle), 8 .. 16 (the measurement).  A file
// writes its launch once, as a generic lambda.
template <int RULE, class F>
static void gadget_for_ldr(int64_t ldr, F&& f) {
    if constexpr (RULE == RULE_EC)
        ldr_dispatch<3, GF2_CIRCUIT_MAX_LDR>(ldr, f);
    else
        ldr_dispatch<FT_MIN_LDR, GF2_FT_MAX_LDR>(ldr, f);
}

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

// The wavefront tally of the counting kernels.  The bin (a configuration class's F counts in LDS) is wave-uniform, so one lane adds
// the wavefront's count of an indicator ...
__device__ __forceinline__ void gadget_add_votes(unsigned int* bin, bool first_lane, bool vote) {
    const u64 votes = __ballot(vote);
    if (votes != 0ull && first_lane) atomicAdd(bin, (unsigned int)__popcll(votes));
}

// ... or of a sum field below 2^BITS among the accepted lanes.
template <int BITS>
__device__ __forceinline__ void gadget_add_sum(unsigned int* bin, bool first_lane, bool acc, unsigned int value) {
    unsigned int sum = 0;
#pragma unroll
    for (int b = 0; b < BITS; ++b) sum += (unsigned int)__popcll(__ballot(acc && ((value >> b) & 1u))) << b;
    if (sum != 0u && first_lane) atomicAdd(bin, sum);
}

// Fields 1 .. 7 of the cycle's counts from what ec_chain gave the accepted lanes (acc) ...
__device__ __forceinline__ void ec_add_tally(unsigned int* bin, bool first_lane, bool acc, const bool (&flip)[2], const bool (&miss)[2],
                                             const unsigned int (&unmatched)[2]) {
    gadget_add_votes(&bin[1], first_lane, acc && flip[0]);
    gadget_add_votes(&bin[2], first_lane, acc && flip[1]);
    gadget_add_votes(&bin[3], first_lane, acc && (flip[0] || flip[1]));
    gadget_add_votes(&bin[4], first_lane, acc && miss[0]);
    gadget_add_votes(&bin[5], first_lane, acc && miss[1]);
    gadget_add_sum<3>(&bin[6], first_lane, acc, unmatched[0]);                     // <= GF2_EC_MAX_ROUNDS = 6
    gadget_add_sum<3>(&bin[7], first_lane, acc, unmatched[1]);
}

// ... and fields 1 .. 6 of the measurement's from what ft_walk gave them.
__device__ __forceinline__ void ft_add_tally(unsigned int* bin, bool first_lane, bool acc, unsigned int wrong_trials, unsigned int first_wrong,
                                             const unsigned int (&unmatched)[2], unsigned int trials) {
    gadget_add_votes(&bin[1], first_lane, acc && 2 * wrong_trials > trials);
    gadget_add_sum<4>(&bin[2], first_lane, acc, wrong_trials);                     // <= trials <= 15 steps
    gadget_add_votes(&bin[3], first_lane, acc && first_wrong != 0u);
    gadget_add_votes(&bin[4], first_lane, acc && wrong_trials != 0u && wrong_trials != trials);
    gadget_add_sum<4>(&bin[5], first_lane, acc, unmatched[0]);                     // <= nsteps <= 15
    gadget_add_sum<4>(&bin[6], first_lane, acc, unmatched[1]);
}
