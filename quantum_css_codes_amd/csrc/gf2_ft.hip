// Fault Monte-Carlo of the fault-tolerant logical measurement (DESIGN.md "Logical measurement"): the one-qubit program that
// ftqc.rewrite_program (ftqc.py:76-95) emits -- verified encoding, logical Paulis each followed by a round of error correction, then
// CSSCode.measure (css_code.py:542-589): 2t + 1 noisy measurements with a round of error correction after each and a majority vote --
// under circuit-level faults.  As in gf2_ec.hip, corrections are recorded and never applied, so one effect table carries the physics
// and a sample is the gather loop of circuit_kernel (gf2_circuit_dev.h, unchanged), lane = sample.
//
// The outcome words are [step 0 .. nsteps - 1] [flag words], 8 <= LDR <= GF2_FT_MAX_LDR of them.  A step is an EC step (key_x in the
// low half of its word, key_z in the high half) or, where measure_mask has its bit, a MEASURE step (key_x, and the measured
// z_operator parity on bit 31).  A sample with a flag bit set is rejected.  An accepted one walks its steps in order with one record
// of known errors per side (syndrome K, operator parity P): corrections and measurements share data.x_errors, so a trial's bit is
// read against everything recorded up to and including its own key.  The walk is fully unrolled over the constant word index s with
// the uniform guards s < nsteps and (measure_mask >> s) & 1, and acceptance is an OR over constant w selected by w >= nsteps: out[]
// never takes a run-time index (gf2_ec.hip says why: it would go to scratch).  K, P, the count of wrong trials and the per-lane
// tallies stay in registers.
//
// LDS per workgroup: the sampler's two inverse-CDF tables, the taken maps and the seven counts.  The effect table is always read
// through L2: the smallest program's (Steane, no gates: 2 * 1630 * 8 words) is ten times CIRC_EFF_LDS_BYTES.  A workgroup does
// at most 7 LDS atomics per lane with something to add and 7 global atomics.
#include "gf2_internal.h"
#include "gf2_gadget_dev.h"

#define FT_FIELDS GF2_FT_FIELDS
#define FT_LAUNCH_SAMPLES (1ll << 36)          // per launch: keeps a lane's and a workgroup's 32-bit tallies far from wrapping

enum { FT_STORE = 0, FT_TALLY = 1 };

struct FtArgs {
    const u64* eff;
    int locations;
    u64 seed;
    int64_t first_sample, count;
    SegTables th;
    // store
    u64* out;
    int64_t ldo;
    // tally
    int nsteps, trials, first_measure;         // steps; set bits of measure_mask; its lowest set bit
    unsigned int measure_mask;
    u64 mask[2];                               // [0]: the r_2 bits of key_x, [1]: the r_1 bits of key_z
    int kwx, kwz;                              // 1 and 1 (CircuitTables reads them)
    HashTab tab[2];                            // [0]: parity_check_c2's table (key_x), [1]: parity_check_c1's (key_z)
    const unsigned char* flips[2];             // operator . correction of every table entry
    u64* counts;
};

template <int LDR, int EPI>
__global__ __launch_bounds__(CIRC_THREADS) void ft_kernel(FtArgs a) {
    extern __shared__ u64 ft_lds[];
    u64* cdf_lds = ft_lds;                                                         // [2][GF2_SEG_CDF]
    unsigned int* taken = (unsigned int*)(ft_lds + 2 * GF2_SEG_CDF);
    unsigned int* bins = taken + CIRC_THREADS * CIRC_TAKEN_STRIDE;                 // FT_FIELDS
    for (int i = threadIdx.x; i < 2 * GF2_SEG_CDF; i += blockDim.x)
        if (a.th.nseg > 1 || i >= GF2_SEG_CDF) cdf_lds[i] = a.th.cdf[i];            // (one segment: only the last one's table is read)
    if (EPI == FT_TALLY && threadIdx.x < FT_FIELDS) bins[threadIdx.x] = 0;
    __syncthreads();
    unsigned int* mine = taken + threadIdx.x * CIRC_TAKEN_STRIDE;
    unsigned int local[FT_FIELDS] = {0, 0, 0, 0, 0, 0, 0};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += stride) {
        const u64 ks = sample_key(a.seed, (u64)(a.first_sample + i));
        u64 out[LDR];
#pragma unroll
        for (int w = 0; w < LDR; ++w) out[w] = 0;
        circuit_gather<LDR>(a.th, cdf_lds, a.eff, mine, ks, out);
        if constexpr (EPI == FT_STORE) {
#pragma unroll
            for (int w = 0; w < LDR; ++w) a.out[i * a.ldo + w] = out[w];
        } else {
            u64 flags = 0;
#pragma unroll
            for (int w = 1; w < LDR; ++w) flags |= w >= a.nsteps ? out[w] : 0ull;  // (word 0 is a step's: nsteps >= 1)
            if (flags) continue;                                                   // a verification fired: the attempt is repeated
            u64 K[2] = {0, 0};                                                     // syndrome of the errors recorded so far, per side
            unsigned int P[2] = {0, 0};                                            // ... and their operator parity
            unsigned int wrong_trials = 0, first_wrong = 0;
#pragma unroll
            for (int s = 0; s < LDR - 1; ++s) {
                if (s < a.nsteps) {
                    const bool measure = (a.measure_mask >> s) & 1u;
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        if (c == 0 || !measure) {                                  // a measurement corrects data.x_errors only
                            const u64 v = ((out[s] >> (32 * c)) & a.mask[c]) ^ K[c];
                            const u64 slot = hash_find<1>(a.tab[c], 0ull, v);
                            if (slot == ~0ull) {
                                local[5 + c] += 1;                                 // css_code.py:655-657: no match, nothing recorded
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
            local[0] += 1;
            local[1] += 2 * wrong_trials > (unsigned int)a.trials;
            local[2] += wrong_trials;
            local[3] += first_wrong;
            local[4] += wrong_trials != 0 && wrong_trials != (unsigned int)a.trials;
        }
    }
    if constexpr (EPI == FT_TALLY) {
#pragma unroll
        for (int k = 0; k < FT_FIELDS; ++k)
            if (local[k]) atomicAdd(&bins[k], local[k]);
        __syncthreads();
        if (threadIdx.x < FT_FIELDS && bins[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (u64)bins[threadIdx.x]);
    }
}

template <int EPI>
static int ft_launch(gf2_ctx* ctx, const gf2_circuit* circ, const FtArgs& a) {
    const size_t lds = (size_t)2 * GF2_SEG_CDF * 8 + (size_t)CIRC_THREADS * CIRC_TAKEN_STRIDE * 4 + 8 * 4;
    int64_t blocks = gf2_cdiv(a.count, CIRC_THREADS * 16);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
    gadget_for_ldr<RULE_FT>(circ->ldr, [&](auto ldr) {
        hipLaunchKernelGGL((ft_kernel<decltype(ldr)::value, EPI>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    });
    GF2_TRY(gf2_prof_end(ctx));
    GF2_HIP(hipGetLastError());
    return GF2_OK;
}

extern "C" {

int gf2_ft_circuit_create(gf2_ctx* ctx, const uint64_t* eff, int64_t locations, int64_t ldr, gf2_circuit** circuit_out) {
    return gf2_circuit_create_upto("gf2_ft_circuit_create", ctx, eff, locations, ldr, GF2_FT_MAX_LDR, circuit_out);
}

int gf2_ft_outcomes_dev(gf2_ctx* ctx, const gf2_circuit* circuit, uint64_t seed, int64_t first_sample, int64_t count, double p_x,
                        double p_y, double p_z, uint64_t* out_dev, int64_t ldo) {
    const char* who = "gf2_ft_outcomes_dev";
    if (!ctx || !circuit) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (circuit->ldr < FT_MIN_LDR)                                        // (the same words from circuit_kernel's store epilogue)
        return gf2_circuit_outcomes_dev(ctx, circuit, seed, first_sample, count, p_x, p_y, p_z, out_dev, ldo);
    if (circuit->ldr > GF2_FT_MAX_LDR) GF2_FAIL(GF2_E_ARG, "%s: needs ldr <= %d words per sample, got %lld", who, GF2_FT_MAX_LDR, (long long)circuit->ldr);
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "%s: negative range", who);
    if (ldo < circuit->ldr) GF2_FAIL(GF2_E_ARG, "%s: ldo must be at least the circuit's %lld words", who, (long long)circuit->ldr);
    GF2_TRY(check_probabilities(p_x, p_y, p_z));
    if (count == 0) return GF2_OK;
    if (!out_dev) GF2_FAIL(GF2_E_ARG, "%s: null buffer", who);
    GF2_TRY(gf2_ctx_activate(ctx));
    FtArgs a = {};
    GF2_TRY(gf2_seg_tables(ctx, p_x, p_y, p_z, circuit->locations, &a.th));
    a.eff = circuit->eff_dev;
    a.locations = (int)circuit->locations;
    a.seed = seed;
    a.first_sample = first_sample;
    a.count = count;
    a.out = (u64*)out_dev;
    a.ldo = ldo;
    return ft_launch<FT_STORE>(ctx, circuit, a);
}

int gf2_mc_ft_decode(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1, const uint64_t* keys1,
                     const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                     uint64_t seed, int64_t first_sample, int64_t count, double p_x, double p_y, double p_z, uint64_t* counts_out) {
    const char* who = "gf2_mc_ft_decode";
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    FtArgs a = {};
    GF2_TRY(ft_rule_args(who, circuit, nsteps, measure_mask, r1, r2, &a));
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "%s: negative range", who);
    GF2_TRY(check_probabilities(p_x, p_y, p_z));
    GF2_TRY(gf2_ctx_activate(ctx));
    for (int k = 0; k < FT_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    GF2_TRY(gf2_seg_tables(ctx, p_x, p_y, p_z, circuit->locations, &a.th));
    a.eff = circuit->eff_dev;
    a.locations = (int)circuit->locations;
    a.seed = seed;
    CircuitTables tables(ctx);
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, FT_FIELDS, &a));
    a.counts = tables.counts_dev;
    for (int64_t done = 0; done < count; done += FT_LAUNCH_SAMPLES) {
        a.first_sample = first_sample + done;
        a.count = count - done < FT_LAUNCH_SAMPLES ? count - done : FT_LAUNCH_SAMPLES;
        GF2_TRY(ft_launch<FT_TALLY>(ctx, circuit, a));
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, FT_FIELDS * 8);
}

}  // extern "C"
