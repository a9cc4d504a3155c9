// Fault Monte-Carlo of the error-correction cycle (DESIGN.md "Error-correction cycle"): Steane's gadget, CSSCode.error_correct
// (css_code.py:436-470), `rounds` times under circuit-level faults.  Corrections are recorded, never applied (CodeBlock.x_errors), so
// everything but the table lookups is linear over GF(2): one effect table for the whole gadget (gf2_circuit_effects_timed: RESET and
// timed outcome rows) carries the physics, and a sample is the gather loop of circuit_kernel (gf2_circuit_dev.h), lane = sample.
//
// What is new is the epilogue, a chain instead of one lookup.  The outcome words are [final data frame] [round 1 .. rounds] [flag
// words]; both keys of a frame share a word (r <= 31: key_x in the low half, key_z in the high half, the final frame's two parity bits
// on bits 31 and 63).  A sample whose flag words are not all zero is rejected: the reference repeats a preparation until its two
// verifications come out clean, and one attempt per preparation with post-selection has the accepted attempts' distribution.  An
// accepted sample decodes round t's key relative to the syndrome K of what earlier rounds recorded, then judges the final frame
// against the record.  The chain is unrolled to GF2_EC_MAX_ROUNDS with the uniform guard t <= rounds and constant indices into
// out[], and acceptance is an OR over constant w selected by w > rounds: a run-time index would put out[] into scratch.
//
// LDS per workgroup as circuit_kernel's: the sampler's two inverse-CDF tables, the effect table when it fits CIRC_EFF_LDS_BYTES, the
// taken maps, and the eight counts.  Per-lane tallies stay in registers; a workgroup does 8 LDS atomics per lane with something to
// add and 8 global atomics.
#include "gf2_internal.h"
#include "gf2_gadget_dev.h"

#define EC_FIELDS GF2_EC_FIELDS
#define EC_MAX_ROUNDS GF2_EC_MAX_ROUNDS
#define EC_LAUNCH_SAMPLES (1ll << 36)          // per launch: keeps a lane's and a workgroup's 32-bit tallies far from wrapping

struct EcArgs {
    const u64* eff;
    int locations;
    u64 seed;
    int64_t first_sample, count;
    SegTables th;
    int rounds;
    u64 mask[2];                               // [0]: the r_2 bits of key_x, [1]: the r_1 bits of key_z
    int kwx, kwz;                              // 1 and 1 (CircuitTables reads them)
    HashTab tab[2];                            // [0]: parity_check_c2's table (key_x), [1]: parity_check_c1's (key_z)
    const unsigned char* flips[2];             // operator . correction of every table entry
    u64* counts;
};

template <int LDR, bool STAGED>
__global__ __launch_bounds__(CIRC_THREADS) void ec_kernel(EcArgs a) {
    extern __shared__ u64 ec_lds[];
    u64* cdf_lds = ec_lds;                                                         // [2][GF2_SEG_CDF]
    u64* eff_lds = ec_lds + 2 * GF2_SEG_CDF;
    unsigned int* taken = (unsigned int*)(eff_lds + (STAGED ? 2 * a.locations * LDR : 0));
    unsigned int* bins = taken + CIRC_THREADS * CIRC_TAKEN_STRIDE;                 // EC_FIELDS
    for (int i = threadIdx.x; i < 2 * GF2_SEG_CDF; i += blockDim.x)
        if (a.th.nseg > 1 || i >= GF2_SEG_CDF) cdf_lds[i] = a.th.cdf[i];            // (one segment: only the last one's table is read)
    if (STAGED)
        for (int i = threadIdx.x; i < 2 * a.locations * LDR; i += blockDim.x) eff_lds[i] = a.eff[i];
    if (threadIdx.x < EC_FIELDS) bins[threadIdx.x] = 0;
    __syncthreads();
    const u64* eff = STAGED ? eff_lds : a.eff;
    unsigned int* mine = taken + threadIdx.x * CIRC_TAKEN_STRIDE;
    unsigned int local[EC_FIELDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += stride) {
        const u64 ks = sample_key(a.seed, (u64)(a.first_sample + i));
        u64 out[LDR];
#pragma unroll
        for (int w = 0; w < LDR; ++w) out[w] = 0;
        circuit_gather<LDR>(a.th, cdf_lds, eff, mine, ks, out);
        u64 flags = 0;
#pragma unroll
        for (int w = 2; w < LDR; ++w) flags |= w > a.rounds ? out[w] : 0ull;       // (word 1 is a round's: rounds >= 1)
        if (flags) continue;                                                       // a verification fired: the attempt is repeated
        bool flip[2], miss[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            u64 K = 0;                                                             // syndrome of the errors recorded so far
            unsigned int P = 0;                                                    // ... and their operator parity
#pragma unroll
            for (int t = 1; t <= EC_MAX_ROUNDS; ++t) {
                if (t <= LDR - 2 && t <= a.rounds) {
                    const u64 s = ((out[t < LDR ? t : 0] >> (32 * c)) & a.mask[c]) ^ K;
                    const u64 slot = hash_find<1>(a.tab[c], 0ull, s);
                    if (slot == ~0ull) {
                        local[6 + c] += 1;                                         // css_code.py:655-657: no match, nothing recorded
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
        local[0] += 1;
        local[1] += flip[0];
        local[2] += flip[1];
        local[3] += flip[0] | flip[1];
        local[4] += miss[0];
        local[5] += miss[1];
    }
#pragma unroll
    for (int k = 0; k < EC_FIELDS; ++k)
        if (local[k]) atomicAdd(&bins[k], local[k]);
    __syncthreads();
    if (threadIdx.x < EC_FIELDS && bins[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (u64)bins[threadIdx.x]);
}

static int ec_launch(gf2_ctx* ctx, const gf2_circuit* circ, const EcArgs& a) {
    size_t lds;
    const bool staged = circuit_staged(circ, true, (size_t)2 * GF2_SEG_CDF * 8 + (size_t)CIRC_THREADS * CIRC_TAKEN_STRIDE * 4 + EC_FIELDS * 4, &lds);
    int64_t blocks = gf2_cdiv(a.count, CIRC_THREADS * 16);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
    gadget_for_ldr<RULE_EC>(circ->ldr, [&](auto ldr) {
        constexpr int LDR = decltype(ldr)::value;
        if (staged)
            hipLaunchKernelGGL((ec_kernel<LDR, true>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
        else
            hipLaunchKernelGGL((ec_kernel<LDR, false>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    });
    GF2_TRY(gf2_prof_end(ctx));
    GF2_HIP(hipGetLastError());
    return GF2_OK;
}

extern "C" {

int gf2_mc_ec_decode(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                     int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed,
                     int64_t first_sample, int64_t count, double p_x, double p_y, double p_z, uint64_t* counts_out) {
    const char* who = "gf2_mc_ec_decode";
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    EcArgs a = {};
    GF2_TRY(ec_rule_args(who, circuit, rounds, r1, r2, &a));
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "%s: negative range", who);
    GF2_TRY(check_probabilities(p_x, p_y, p_z));
    GF2_TRY(gf2_ctx_activate(ctx));
    for (int k = 0; k < EC_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    GF2_TRY(gf2_seg_tables(ctx, p_x, p_y, p_z, circuit->locations, &a.th));
    a.eff = circuit->eff_dev;
    a.locations = (int)circuit->locations;
    a.seed = seed;
    CircuitTables tables(ctx);
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, EC_FIELDS, &a));
    a.counts = tables.counts_dev;
    for (int64_t done = 0; done < count; done += EC_LAUNCH_SAMPLES) {
        a.first_sample = first_sample + done;
        a.count = count - done < EC_LAUNCH_SAMPLES ? count - done : EC_LAUNCH_SAMPLES;
        GF2_TRY(ec_launch(ctx, circuit, a));
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, EC_FIELDS * 8);
}

}  // extern "C"
