// Direct Monte-Carlo of the two post-selected gadgets under gate-level faults (DESIGN.md section 5e "Direct Monte-Carlo under
// gate-level faults", include/gf2hip.h "direct Monte-Carlo ... under gate-level faults"): every gate of the error-correction cycle or
// of a rewritten one-qubit program fails on its own -- a one-operand gate with probability p_1 and one of 3 kinds, a CNOT as one event
// with probability p_2 and one of 15 -- and the sample is judged by the gadget's own tally rule, post-selection included.  No
// truncation in the number of faulty gates: what the strata of gf2_gate_enumerate.hip and gf2_gate_strata.hip leave out beyond 16
// faulty gates is drawn here with its own probability.
//
// The draw is circuit_gather's (gf2_circuit_dev.h) run once per class of sites: lane = sample, a class cut into segments of 512
// sites, one draw and one inverse-CDF look-up per segment, Floyd's rule against the lane's 512-bit "taken" map in LDS, which a segment
// touches only when it has more than one pick and which serves both classes in turn.  A pick's kind is the sampled strata's
// (1 + ((lo * radix) >> 32)); it reads its first location from site_loc (LDS beside the effect table when staged, L2 otherwise) and
// XORs the effects its kind mask names: up to two for a one-operand gate, up to four for a CNOT.  out[] never takes a run-time index.
//
// LDS per workgroup: four inverse-CDF tables (whole and last segment of each class, 4 x 513 words), the effect table and the site
// table when the former fits CIRC_EFF_LDS_BYTES, the taken maps and the counts: below 64 KiB (gate_mc_launch_lds).  The tally is ec_kernel's
// / ft_kernel's: per-lane registers, one LDS atomic per field with something to add, one global atomic per non-zero field and
// workgroup.
//
// 32-bit tallies: a launch covers at most GATE_MC_LAUNCH_SAMPLES = 2^36 samples on 4096 workgroups, 2^24 per workgroup; a sample adds
// at most GATE_MC_MAX_ADD = 15 to a field (unmatched keys of 15 steps), so a lane's register and a workgroup's bin stay below 2^28.
#include "gf2_internal.h"
#include "gf2_circuit_dev.h"
#include "gf2_gadget_dev.h"

#define GATE_MC_LAUNCH_SAMPLES (1ll << 36)
#define GATE_MC_MAX_BLOCKS 4096
#define GATE_MC_MAX_ADD 15
#define GATE_MC_CDF_WORDS (4 * GF2_SEG_CDF)    // [class][whole segments, last segment][GF2_SEG_CDF]
static_assert(GATE_MC_LAUNCH_SAMPLES / GATE_MC_MAX_BLOCKS * GATE_MC_MAX_ADD < (1ll << 32), "a workgroup's 32-bit bins must hold a whole launch");
static_assert(GF2_FT_MAX_LDR - 1 <= GATE_MC_MAX_ADD && GF2_EC_MAX_ROUNDS <= GATE_MC_MAX_ADD, "a sum field's value per sample");
static_assert(GF2_CIRCUIT_MAX_LOCATIONS / GF2_SEG_BITS <= 2048 && GF2_GATE_MC_SLOT_ONE >= 2048 &&
                  GF2_GATE_MC_SLOT_CNOT >= GF2_GATE_MC_SLOT_ONE + 2048,
              "the slots of the location sampler and of the two classes are disjoint");
// A staged effect table has at most CIRC_EFF_LDS_BYTES / (16 * 3) locations (3 words per effect at least), and no more sites.
static_assert(GATE_MC_CDF_WORDS * 8 + CIRC_EFF_LDS_BYTES + CIRC_EFF_LDS_BYTES / 48 * 4 + CIRC_THREADS * CIRC_TAKEN_STRIDE * 4 + 8 * 4 <= 65536,
              "the dynamic LDS of a staged launch stays below 64 KiB");

// gf2_host.cpp: the argument rules of the site table and of the rates and the range, shared with the host statement
int gf2_gate_check_sites(const char* who, int64_t locations, const int32_t* site_loc, int64_t n1, int64_t n2);
int gf2_gate_check_mc(const char* who, double p1, double p2, int64_t first_sample, int64_t count);

struct GateMcArgs {
    const u64* eff;
    const int* site_loc;                       // n1 + n2 first locations, the one-operand sites first
    const u64* cdf;                            // GATE_MC_CDF_WORDS: the call's four inverse-CDF tables
    int locations, n1, n2;
    u64 seed;
    int64_t first_sample, count;
    int rounds;                                // the cycle
    int nsteps, trials, first_measure;         // the measurement: steps; set bits of measure_mask; its lowest set bit
    unsigned int measure_mask;
    u64 mask[2];                               // [0]: the r_2 bits of key_x, [1]: the r_1 bits of key_z
    int kwx, kwz;                              // 1 and 1 (CircuitTables reads them)
    HashTab tab[2];                            // [0]: parity_check_c2's table (key_x), [1]: parity_check_c1's (key_z)
    const unsigned char* flips[2];             // operator . correction of every table entry
    u64* counts;
};

// The faults of one class of sites of sample `ks` XOR-ed into out[]: circuit_gather's loop over the m sites from site_base on
// (cdf_lds: the class's two staged tables).  A position is below nb, so its site is below site_base + m <= n1 + n2, and its first
// location and the effects its mask names lie inside the table (the site table is checked on the host).
template <int LDR, bool CNOT>
__device__ __forceinline__ void gate_class_gather(int m, int site_base, const u64* cdf_lds, const u64* eff, const int* site_loc,
                                                  unsigned int* mine, u64 ks, u64 (&out)[LDR]) {
    const int nseg = (m + GF2_SEG_BITS - 1) / GF2_SEG_BITS;
    for (int s = 0; s < nseg; ++s) {
        const bool last = s == nseg - 1;
        const int nb = last ? m - s * GF2_SEG_BITS : GF2_SEG_BITS;
        const u64 d = segment_draw(ks, (u64)((CNOT ? GF2_GATE_MC_SLOT_CNOT : GF2_GATE_MC_SLOT_ONE) + s));
        const int K = error_count(d, nb, cdf_lds + (last ? GF2_SEG_CDF : 0));
        if (K > 1)
            for (int w = 0; w < (nb + 31) >> 5; ++w) mine[w] = 0;
        for (int k = 0; k < K; ++k) {
            const u64 v = mix64(d + GF2_GOLDEN * (u64)(k + 1));
            const u64 hi = v >> 32, lo = v & 0xFFFFFFFFull;
            const unsigned int j = (unsigned int)(nb - K + k);
            const unsigned int t = (unsigned int)((hi * (u64)(j + 1u)) >> 32);
            unsigned int pos = t;
            if (K > 1) {                                                       // Floyd's rule: a candidate already taken -> j
                if ((mine[t >> 5] >> (t & 31u)) & 1u) pos = j;
                mine[pos >> 5] |= 1u << (pos & 31u);
            }
            const unsigned int kappa = 1u + (unsigned int)((lo * (CNOT ? 15ull : 3ull)) >> 32);
            const u64* e = eff + (size_t)(2u * (unsigned int)site_loc[site_base + s * GF2_SEG_BITS + (int)pos]) * LDR;
            if (kappa & 1u) {
#pragma unroll
                for (int w = 0; w < LDR; ++w) out[w] ^= e[w];
            }
            if (kappa & 2u) {
#pragma unroll
                for (int w = 0; w < LDR; ++w) out[w] ^= e[LDR + w];
            }
            if (CNOT) {                                                        // the target's two effects: location l + 1
                if (kappa & 4u) {
#pragma unroll
                    for (int w = 0; w < LDR; ++w) out[w] ^= e[2 * LDR + w];
                }
                if (kappa & 8u) {
#pragma unroll
                    for (int w = 0; w < LDR; ++w) out[w] ^= e[3 * LDR + w];
                }
            }
        }
    }
}

template <int LDR, int RULE, bool STAGED = false>
__global__ __launch_bounds__(CIRC_THREADS) void gate_mc_kernel(GateMcArgs a) {
    constexpr int F = RULE == RULE_EC ? GF2_EC_FIELDS : GF2_FT_FIELDS;
    extern __shared__ u64 gate_mc_lds[];
    u64* cdf_lds = gate_mc_lds;                                                    // GATE_MC_CDF_WORDS
    u64* eff_lds = cdf_lds + GATE_MC_CDF_WORDS;
    int* sites_lds = (int*)(eff_lds + (STAGED ? 2 * a.locations * LDR : 0));       // n1 + n2 when staged
    unsigned int* taken = (unsigned int*)(sites_lds + (STAGED ? a.n1 + a.n2 : 0));
    unsigned int* bins = taken + CIRC_THREADS * CIRC_TAKEN_STRIDE;                 // F
    for (int i = threadIdx.x; i < GATE_MC_CDF_WORDS; i += blockDim.x) cdf_lds[i] = a.cdf[i];
    if (STAGED) {
        for (int i = threadIdx.x; i < 2 * a.locations * LDR; i += blockDim.x) eff_lds[i] = a.eff[i];
        for (int i = threadIdx.x; i < a.n1 + a.n2; i += blockDim.x) sites_lds[i] = a.site_loc[i];
    }
    if (threadIdx.x < F) bins[threadIdx.x] = 0;
    __syncthreads();
    const u64* eff = STAGED ? eff_lds : a.eff;
    const int* site_loc = STAGED ? sites_lds : a.site_loc;
    unsigned int* mine = taken + threadIdx.x * CIRC_TAKEN_STRIDE;
    unsigned int local[F];
#pragma unroll
    for (int k = 0; k < F; ++k) local[k] = 0;
    unsigned int unmatched[2] = {0, 0};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += stride) {
        const u64 ks = sample_key(a.seed, (u64)(a.first_sample + i));
        u64 out[LDR];
#pragma unroll
        for (int w = 0; w < LDR; ++w) out[w] = 0;
        gate_class_gather<LDR, false>(a.n1, 0, cdf_lds, eff, site_loc, mine, ks, out);
        gate_class_gather<LDR, true>(a.n2, a.n1, cdf_lds + 2 * GF2_SEG_CDF, eff, site_loc, mine, ks, out);
        const u64 flags = RULE == RULE_EC ? ec_flag_or<LDR>(a, out) : ft_flag_or<LDR>(a, out);
        if (flags) continue;                                                       // a verification fired: the attempt is repeated
        local[0] += 1;
        if constexpr (RULE == RULE_EC) {
            bool flip[2], miss[2];
            ec_chain<LDR>(a, out, flip, miss, unmatched);
            local[1] += flip[0];
            local[2] += flip[1];
            local[3] += flip[0] | flip[1];
            local[4] += miss[0];
            local[5] += miss[1];
        } else {
            unsigned int wrong_trials = 0, first_wrong = 0;
            ft_walk<LDR>(a, out, wrong_trials, first_wrong, unmatched);
            local[1] += 2 * wrong_trials > (unsigned int)a.trials;
            local[2] += wrong_trials;
            local[3] += first_wrong;
            local[4] += wrong_trials != 0u && wrong_trials != (unsigned int)a.trials;
        }
    }
    local[F - 2] = unmatched[0];
    local[F - 1] = unmatched[1];
#pragma unroll
    for (int k = 0; k < F; ++k)
        if (local[k]) atomicAdd(&bins[k], local[k]);
    __syncthreads();
    if (threadIdx.x < F && bins[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (u64)bins[threadIdx.x]);
}

namespace {
struct DevBuffer {                                                                      // a device buffer of the call's, freed with it
    gf2_ctx* ctx;
    void* dev = nullptr;
    explicit DevBuffer(gf2_ctx* c) : ctx(c) {}
    ~DevBuffer() { (void)gf2_dev_free(ctx, dev); }
};
}  // namespace

// The dynamic LDS of a launch and whether it stages the effect table (and the site table beside it).
static bool gate_mc_launch_lds(const gf2_circuit* circ, bool allowed, int64_t sites, size_t* lds) {
    const bool staged = circuit_staged(circ, allowed, (size_t)GATE_MC_CDF_WORDS * 8 + (size_t)CIRC_THREADS * CIRC_TAKEN_STRIDE * 4 + 8 * 4, lds);
    if (staged) *lds += (size_t)sites * 4;                                              // (sites <= locations: see the static_assert)
    return staged;
}

// The samples of a call whose circuit and layout are checked: the four inverse-CDF tables, the hash tables and the site table made
// for this call alone, the range cut into launches of at most GATE_MC_LAUNCH_SAMPLES samples, the counts back once.
template <int RULE>
static int gate_mc(const char* who, gf2_ctx* ctx, const gf2_circuit* circuit, GateMcArgs& a, const uint64_t* keys1, const uint8_t* flips1,
                   int64_t entries1, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, const int32_t* site_loc, int64_t n1,
                   int64_t n2, uint64_t seed, int64_t first_sample, int64_t count, double p1, double p2, uint64_t* counts_out) {
    constexpr int F = RULE == RULE_EC ? GF2_EC_FIELDS : GF2_FT_FIELDS;
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    GF2_TRY(gf2_gate_check_sites(who, circuit->locations, site_loc, n1, n2));
    GF2_TRY(gf2_gate_check_mc(who, p1, p2, first_sample, count));
    GF2_TRY(gf2_ctx_activate(ctx));
    for (int k = 0; k < F; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    u64 cdf[GATE_MC_CDF_WORDS];
    const int64_t m[2] = {n1, n2};
    const uint64_t T[2] = {gf2_quantise(p1), gf2_quantise(p2)};
    for (int c = 0; c < 2; ++c) {
        const int nb_last = m[c] > 0 ? (int)(m[c] - (m[c] - 1) / GF2_SEG_BITS * GF2_SEG_BITS) : 0;
        binomial_cdf_table(T[c], GF2_SEG_BITS, cdf + (2 * c) * GF2_SEG_CDF, GF2_SEG_CDF);
        binomial_cdf_table(T[c], nb_last, cdf + (2 * c + 1) * GF2_SEG_CDF, GF2_SEG_CDF);
    }
    CircuitTables tables(ctx);
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, F, &a));
    DevBuffer sites(ctx), cdf_dev(ctx);
    GF2_TRY(gf2_dev_alloc(ctx, (size_t)(n1 + n2) * 4, &sites.dev));
    GF2_TRY(gf2_h2d(ctx, sites.dev, site_loc, (size_t)(n1 + n2) * 4));
    GF2_TRY(gf2_dev_alloc(ctx, sizeof cdf, &cdf_dev.dev));
    GF2_TRY(gf2_h2d(ctx, cdf_dev.dev, cdf, sizeof cdf));
    a.eff = circuit->eff_dev;
    a.site_loc = (const int*)sites.dev;
    a.cdf = (const u64*)cdf_dev.dev;
    a.locations = (int)circuit->locations;
    a.n1 = (int)n1;
    a.n2 = (int)n2;
    a.seed = seed;
    a.counts = tables.counts_dev;
    size_t lds;
    const bool staged = gate_mc_launch_lds(circuit, RULE == RULE_EC, n1 + n2, &lds);           // (the measurement's tables never fit)
    for (int64_t done = 0; done < count; done += GATE_MC_LAUNCH_SAMPLES) {
        a.first_sample = first_sample + done;
        a.count = count - done < GATE_MC_LAUNCH_SAMPLES ? count - done : GATE_MC_LAUNCH_SAMPLES;
        int64_t blocks = gf2_cdiv(a.count, CIRC_THREADS * 16);
        if (blocks > GATE_MC_MAX_BLOCKS) blocks = GATE_MC_MAX_BLOCKS;
        if (blocks < 1) blocks = 1;
        GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
        gadget_for_ldr<RULE>(circuit->ldr, [&](auto ldr) {
            constexpr int LDR = decltype(ldr)::value;
            if constexpr (RULE == RULE_EC) {
                if (staged) {
                    hipLaunchKernelGGL((gate_mc_kernel<LDR, RULE, true>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
                    return;
                }
            }
            hipLaunchKernelGGL((gate_mc_kernel<LDR, RULE, false>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
        });
        GF2_TRY(gf2_prof_end(ctx));
        GF2_HIP(hipGetLastError());
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, (size_t)F * 8);
}

extern "C" {

int gf2_mc_ec_decode_gate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1,
                          const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                          int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, uint64_t seed, int64_t first_sample,
                          int64_t count, double p1, double p2, uint64_t* counts_out) {
    const char* who = "gf2_mc_ec_decode_gate";
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GateMcArgs args = {};
    GF2_TRY(ec_rule_args(who, circuit, rounds, r1, r2, &args));
    return gate_mc<RULE_EC>(who, ctx, circuit, args, keys1, flips1, entries1, keys2, flips2, entries2, site_loc, n1, n2, seed, first_sample,
                            count, p1, p2, counts_out);
}

int gf2_mc_ft_decode_gate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                          const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                          const uint8_t* flips2, int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, uint64_t seed,
                          int64_t first_sample, int64_t count, double p1, double p2, uint64_t* counts_out) {
    const char* who = "gf2_mc_ft_decode_gate";
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GateMcArgs args = {};
    GF2_TRY(ft_rule_args(who, circuit, nsteps, measure_mask, r1, r2, &args));
    return gate_mc<RULE_FT>(who, ctx, circuit, args, keys1, flips1, entries1, keys2, flips2, entries2, site_loc, n1, n2, seed, first_sample,
                            count, p1, p2, counts_out);
}

}  // extern "C"
