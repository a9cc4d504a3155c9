// Sampled strata of the two post-selected gadgets (DESIGN.md "Sampled strata of the cycle", "Sampled strata of the measurement"):
// stratified samples of exactly w <= GADGET_STRATUM_MAX faults among the L locations of the error-correction cycle or of a rewritten
// one-qubit program, judged by the gadget's own tally rule, post-selection included.  The weights the exact strata
// (gf2_gadget_enumerate.hip) cannot reach -- weight 3 of the smallest program is 1.8 x 10^10 configurations -- are sampled here, and
// one set of strata serves every physical rate.
//
// Nothing but the combination is new.  The draw is circuit_kernel's stratum mode (gf2_circuit.hip, DESIGN.md "Strata"): lane =
// sample, ONE segment over all L locations whose slot carries the weight, Floyd's rule against the earlier picks, which stay in
// registers -- a fully unrolled loop of GADGET_STRATUM_MAX trips, each under the uniform guard k < weight, constant indices only.
// This file keeps its own text of that loop (stratum_faults is typed on circuit_kernel's argument block, and the two samplers keep
// their own text of the tally rule for the same reason: a shared template moved register counts).  The judgement is the exact
// strata's (gf2_gadget_dev.h): the flag OR, then the chain of ec_kernel or the step walk of ft_kernel on the lane's outcome words;
// out[] never takes a run-time index.
//
// LDS per workgroup of 256 lanes: the effect table when it is the cycle's and fits CIRC_EFF_LDS_BYTES (the measurement's never do:
// every fault then reads its effect through L2), and the F counts.  No CDF table, no taken map.  Per-lane tallies stay in registers;
// a workgroup does at most F LDS atomics per lane with something to add and F global atomics into the stratum's row of the counts.
//
// 32-bit tallies: a launch covers at most GADGET_STRATA_LAUNCH_SAMPLES = 2^36 samples on 4096 x 256 lanes, 2^16 per lane; a sample
// adds at most GADGET_STRATA_MAX_ADD = 15 to a field (unmatched keys of 15 steps), so a lane stays below 2^20 and a workgroup's bin
// below 2^28.
#include "gf2_internal.h"
#include "gf2_circuit_dev.h"
#include "gf2_gadget_dev.h"

#define GADGET_STRATUM_MAX GF2_CIRCUIT_STRATUM_MAX_WEIGHT
#define GADGET_STRATA_LAUNCH_SAMPLES (1ll << 36)
#define GADGET_STRATA_MAX_BLOCKS 4096
#define GADGET_STRATA_MAX_ADD 15
static_assert(GADGET_STRATA_LAUNCH_SAMPLES / GADGET_STRATA_MAX_BLOCKS * GADGET_STRATA_MAX_ADD < (1ll << 32),
              "a workgroup's 32-bit bins (and so every lane's tallies) must hold a whole launch");
static_assert(GF2_FT_MAX_LDR - 1 <= GADGET_STRATA_MAX_ADD && GF2_EC_MAX_ROUNDS <= GADGET_STRATA_MAX_ADD, "a sum field's value per sample");

struct GadgetStrataArgs {
    const u64* eff;
    int locations, weight;
    u64 seed;
    int64_t first_sample, count;
    u64 t_1, t_2;                              // the kind thresholds (stratum_thresholds)
    int rounds;                                // the cycle
    int nsteps, trials, first_measure;         // the measurement: steps; set bits of measure_mask; its lowest set bit
    unsigned int measure_mask;
    u64 mask[2];                               // [0]: the r_2 bits of key_x, [1]: the r_1 bits of key_z
    int kwx, kwz;                              // 1 and 1 (CircuitTables reads them)
    HashTab tab[2];                            // [0]: parity_check_c2's table (key_x), [1]: parity_check_c1's (key_z)
    const unsigned char* flips[2];             // operator . correction of every table entry
    u64* counts;                               // this stratum's F counts
};

// The faults of a stratified sample XOR-ed into out[] (the text of stratum_faults, gf2_circuit.hip, on this file's argument block):
// the at most GADGET_STRATUM_MAX earlier picks in registers, every trip guarded by the uniform k < a.weight.
template <int LDR>
__device__ __forceinline__ void gadget_stratum_faults(const GadgetStrataArgs& a, const u64* eff, u64 ks, u64 (&out)[LDR]) {
    const u64 d = segment_draw(ks, (u64)a.weight);
    unsigned int picks[GADGET_STRATUM_MAX];
#pragma unroll
    for (int k = 0; k < GADGET_STRATUM_MAX; ++k) {
        if (k < a.weight) {
            unsigned int t, kind;
            error_draw(d, k, a.weight, a.locations, a.t_1, a.t_2, &t, &kind);
            bool seen = false;
#pragma unroll
            for (int q = 0; q < k; ++q) seen |= picks[q] == t;
            picks[k] = seen ? (unsigned int)(a.locations - a.weight + k) : t;              // Floyd's rule; below L either way
            const u64* e = eff + (size_t)(2 * picks[k]) * LDR;
            if (kind & 1u) {
#pragma unroll
                for (int w = 0; w < LDR; ++w) out[w] ^= e[w];
            }
            if (kind & 2u) {
#pragma unroll
                for (int w = 0; w < LDR; ++w) out[w] ^= e[LDR + w];
            }
        }
    }
}

template <int LDR, int RULE, bool STAGED = false>
__global__ __launch_bounds__(CIRC_THREADS) void gadget_strata_kernel(GadgetStrataArgs a) {
    constexpr int F = RULE == RULE_EC ? GF2_EC_FIELDS : GF2_FT_FIELDS;
    extern __shared__ u64 gadget_strata_lds[];
    u64* eff_lds = gadget_strata_lds;
    unsigned int* bins = (unsigned int*)(eff_lds + (STAGED ? 2 * a.locations * LDR : 0));   // F
    if (STAGED)
        for (int i = threadIdx.x; i < 2 * a.locations * LDR; i += blockDim.x) eff_lds[i] = a.eff[i];
    if (threadIdx.x < F) bins[threadIdx.x] = 0;
    __syncthreads();
    const u64* eff = STAGED ? eff_lds : a.eff;
    unsigned int local[F];
#pragma unroll
    for (int k = 0; k < F; ++k) local[k] = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += stride) {
        const u64 ks = sample_key(a.seed, (u64)(a.first_sample + i));
        u64 out[LDR];
#pragma unroll
        for (int w = 0; w < LDR; ++w) out[w] = 0;
        gadget_stratum_faults<LDR>(a, eff, ks, out);
        const u64 flags = RULE == RULE_EC ? ec_flag_or<LDR>(a, out) : ft_flag_or<LDR>(a, out);
        if (flags) continue;                                                       // a verification fired: the attempt is repeated
        local[0] += 1;
        if constexpr (RULE == RULE_EC) {
            bool flip[2], miss[2];
            unsigned int unmatched[2] = {0, 0};
            ec_chain<LDR>(a, out, flip, miss, unmatched);
            local[1] += flip[0];
            local[2] += flip[1];
            local[3] += flip[0] | flip[1];
            local[4] += miss[0];
            local[5] += miss[1];
            local[6] += unmatched[0];
            local[7] += unmatched[1];
        } else {
            unsigned int wrong_trials = 0, first_wrong = 0, unmatched[2] = {0, 0};
            ft_walk<LDR>(a, out, wrong_trials, first_wrong, unmatched);
            local[1] += 2 * wrong_trials > (unsigned int)a.trials;
            local[2] += wrong_trials;
            local[3] += first_wrong;
            local[4] += wrong_trials != 0u && wrong_trials != (unsigned int)a.trials;
            local[5] += unmatched[0];
            local[6] += unmatched[1];
        }
    }
#pragma unroll
    for (int k = 0; k < F; ++k)
        if (local[k]) atomicAdd(&bins[k], local[k]);
    __syncthreads();
    if (threadIdx.x < F && bins[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (u64)bins[threadIdx.x]);
}

// The strata of a call whose circuit and layout are checked: the strata arguments checked as gf2_mc_circuit_decode_strata checks
// them, tables made once, every stratum cut into launches of at most GADGET_STRATA_LAUNCH_SAMPLES samples, the counts back once.
template <int RULE>
static int gadget_strata(const char* who, gf2_ctx* ctx, const gf2_circuit* circuit, GadgetStrataArgs& a, const uint64_t* keys1,
                         const uint8_t* flips1, int64_t entries1, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed,
                         int64_t first_sample, int64_t nstrata, const int32_t* weights, const int64_t* counts, double k_x, double k_y,
                         double k_z, uint64_t* counts_out) {
    constexpr int F = RULE == RULE_EC ? GF2_EC_FIELDS : GF2_FT_FIELDS;
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    if (nstrata < 0 || nstrata > GF2_STRATA_MAX || (nstrata && (!weights || !counts)))
        GF2_FAIL(GF2_E_ARG, "%s: needs 0 <= nstrata <= %d and their weights and counts", who, GF2_STRATA_MAX);
    if (first_sample < 0) GF2_FAIL(GF2_E_ARG, "%s: negative range", who);
    int64_t total = 0;
    for (int64_t s = 0; s < nstrata; ++s) {
        if (weights[s] < 0 || weights[s] > GADGET_STRATUM_MAX || weights[s] > circuit->locations)
            GF2_FAIL(GF2_E_ARG, "%s: stratum %lld has weight %d outside [0, min(L = %lld, %d)]", who, (long long)s, (int)weights[s],
                     (long long)circuit->locations, GADGET_STRATUM_MAX);
        if (counts[s] < 0) GF2_FAIL(GF2_E_ARG, "%s: stratum %lld has a negative sample count", who, (long long)s);
        total += counts[s] > 0;
    }
    GF2_TRY(stratum_thresholds(who, k_x, k_y, k_z, &a.t_1, &a.t_2));
    GF2_TRY(gf2_ctx_activate(ctx));
    for (int64_t k = 0; k < F * nstrata; ++k) counts_out[k] = 0;
    if (total == 0) return GF2_OK;
    CircuitTables tables(ctx);
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, F * nstrata, &a));
    a.eff = circuit->eff_dev;
    a.locations = (int)circuit->locations;
    a.seed = seed;
    size_t lds;
    const bool staged = circuit_staged(circuit, RULE == RULE_EC, (size_t)F * 4, &lds);   // (the measurement's tables never fit)
    for (int64_t s = 0; s < nstrata; ++s) {
        a.weight = (int)weights[s];
        a.counts = tables.counts_dev + F * s;
        for (int64_t done = 0; done < counts[s]; done += GADGET_STRATA_LAUNCH_SAMPLES) {
            a.first_sample = first_sample + done;
            a.count = counts[s] - done < GADGET_STRATA_LAUNCH_SAMPLES ? counts[s] - done : GADGET_STRATA_LAUNCH_SAMPLES;
            int64_t blocks = gf2_cdiv(a.count, CIRC_THREADS * 16);
            if (blocks > GADGET_STRATA_MAX_BLOCKS) blocks = GADGET_STRATA_MAX_BLOCKS;
            if (blocks < 1) blocks = 1;
            GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
            gadget_for_ldr<RULE>(circuit->ldr, [&](auto ldr) {
                constexpr int LDR = decltype(ldr)::value;
                if constexpr (RULE == RULE_EC) {
                    if (staged) {
                        hipLaunchKernelGGL((gadget_strata_kernel<LDR, RULE, true>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
                        return;
                    }
                }
                hipLaunchKernelGGL((gadget_strata_kernel<LDR, RULE, false>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
            });
            GF2_TRY(gf2_prof_end(ctx));
            GF2_HIP(hipGetLastError());
        }
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, (size_t)nstrata * F * 8);
}

extern "C" {

int gf2_mc_ec_decode_strata(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1,
                            const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                            int64_t entries2, uint64_t seed, int64_t first_sample, int64_t nstrata, const int32_t* weights,
                            const int64_t* counts, double k_x, double k_y, double k_z, uint64_t* counts_out) {
    const char* who = "gf2_mc_ec_decode_strata";
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GadgetStrataArgs a = {};
    GF2_TRY(ec_rule_args(who, circuit, rounds, r1, r2, &a));
    return gadget_strata<RULE_EC>(who, ctx, circuit, a, keys1, flips1, entries1, keys2, flips2, entries2, seed, first_sample, nstrata,
                                  weights, counts, k_x, k_y, k_z, counts_out);
}

int gf2_mc_ft_decode_strata(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                            const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                            const uint8_t* flips2, int64_t entries2, uint64_t seed, int64_t first_sample, int64_t nstrata,
                            const int32_t* weights, const int64_t* counts, double k_x, double k_y, double k_z, uint64_t* counts_out) {
    const char* who = "gf2_mc_ft_decode_strata";
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GadgetStrataArgs a = {};
    GF2_TRY(ft_rule_args(who, circuit, nsteps, measure_mask, r1, r2, &a));
    return gadget_strata<RULE_FT>(who, ctx, circuit, a, keys1, flips1, entries1, keys2, flips2, entries2, seed, first_sample, nstrata,
                                  weights, counts, k_x, k_y, k_z, counts_out);
}

}  // extern "C"
