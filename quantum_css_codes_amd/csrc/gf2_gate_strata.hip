// Sampled strata of the two post-selected gadgets under gate-level faults (DESIGN.md section 5e "Sampled strata under gate-level
// faults", include/gf2hip.h "sampled strata ... under gate-level faults"): stratified samples of exactly a faulty one-operand gates
// and b faulty CNOTs, a + b <= GATE_STRATUM_MAX, of the error-correction cycle or of a rewritten one-qubit program, judged by the
// gadget's own tally rule, post-selection included, and tallied by the number c of CNOT picks with a two-operand kind.  The weights
// the exact strata (gf2_gate_enumerate.hip) stop at -- four faulty gates -- are continued here, and one set of strata serves every
// (x, y1, y2).
//
// The draw is gadget_strata_kernel's (gf2_gadget_strata.hip) over sites instead of locations: lane = sample, ONE segment whose slot
// 64 + 17 b + a carries the stratum, Floyd's rule per class against the earlier picks, which stay in registers in the unified site
// numbering (the two classes' ranges are disjoint, so one comparison serves both) -- a fully unrolled loop of GATE_STRATUM_MAX
// trips, each under the uniform guard k < a + b, the class of trip k selected by the uniform k < a, constant indices only.  A pick
// reads its first location from site_loc (LDS beside the effect table when staged, L2 otherwise) and XORs the effects its kind mask
// names: up to two for a one-operand gate, up to four for a CNOT.  out[] and the picks never take a run-time index.
//
// The tally.  c differs from lane to lane, so registers indexed by c would go to scratch: an accepted sample adds straight into the
// workgroup's LDS bins [c][F] (at most 17 x 8 dwords), one LDS atomic per field with something to add -- acceptance is low beyond
// weight 2, where these strata matter -- and the workgroup ends with one global atomic per non-zero bin.
//
// 32-bit bins: a launch covers at most GATE_STRATA_LAUNCH_SAMPLES = 2^36 samples on 4096 workgroups, 2^24 per workgroup; a sample
// adds at most GATE_STRATA_MAX_ADD = 15 to a field (unmatched keys of 15 steps), so a bin stays below 2^28.
#include "gf2_internal.h"
#include "gf2_circuit_dev.h"
#include "gf2_gadget_dev.h"

#define GATE_STRATUM_MAX GF2_GATE_STRATUM_MAX_WEIGHT
#define GATE_STRATA_ROWS (GATE_STRATUM_MAX + 1)
#define GATE_STRATA_LAUNCH_SAMPLES (1ll << 36)
#define GATE_STRATA_MAX_BLOCKS 4096
#define GATE_STRATA_MAX_ADD 15
static_assert(GATE_STRATA_LAUNCH_SAMPLES / GATE_STRATA_MAX_BLOCKS * GATE_STRATA_MAX_ADD < (1ll << 32),
              "a workgroup's 32-bit bins must hold a whole launch");
static_assert(GF2_FT_MAX_LDR - 1 <= GATE_STRATA_MAX_ADD && GF2_EC_MAX_ROUNDS <= GATE_STRATA_MAX_ADD, "a sum field's value per sample");
static_assert(GATE_STRATUM_MAX == 16, "the stratum's slot is 64 + 17 b + a");

// gf2_host.cpp: the argument rules of the site table and of one stratum, shared with the host statement
int gf2_gate_check_sites(const char* who, int64_t locations, const int32_t* site_loc, int64_t n1, int64_t n2);
int gf2_gate_check_stratum(const char* who, const char* at, int64_t n1, int64_t n2, int64_t a, int64_t b);

struct GateStrataArgs {
    const u64* eff;
    const int* site_loc;                       // n1 + n2 first locations, the one-operand sites first
    int locations, n1, n2;
    int wa, wb;                                // one-operand picks, CNOT picks of this stratum
    u64 seed;
    int64_t first_sample, count;
    int rounds;                                // the cycle
    int nsteps, trials, first_measure;         // the measurement: steps; set bits of measure_mask; its lowest set bit
    unsigned int measure_mask;
    u64 mask[2];                               // [0]: the r_2 bits of key_x, [1]: the r_1 bits of key_z
    int kwx, kwz;                              // 1 and 1 (CircuitTables reads them)
    HashTab tab[2];                            // [0]: parity_check_c2's table (key_x), [1]: parity_check_c1's (key_z)
    const unsigned char* flips[2];             // operator . correction of every table entry
    u64* counts;                               // this stratum's [GATE_STRATA_ROWS][F] counts
};

// The faults of a stratified sample XOR-ed into out[]; returns c, the number of CNOT picks with a two-operand kind.  A pick's site
// is below n1 + n2 either way (t <= j < n of its class), so its first location and the effects its mask names lie inside the table.
template <int LDR>
__device__ __forceinline__ unsigned int gate_stratum_faults(const GateStrataArgs& a, const u64* eff, const int* site_loc, u64 ks,
                                                            u64 (&out)[LDR]) {
    const int weight = a.wa + a.wb;
    const u64 d = segment_draw(ks, (u64)(64 + 17 * a.wb + a.wa));
    unsigned int picks[GATE_STRATUM_MAX];
    unsigned int c = 0;
#pragma unroll
    for (int k = 0; k < GATE_STRATUM_MAX; ++k) {
        if (k < weight) {
            const bool one = k < a.wa;                                             // (uniform) a one-operand pick
            const u64 v = mix64(d + GF2_GOLDEN * (u64)(k + 1));
            const u64 hi = v >> 32, lo = v & 0xFFFFFFFFull;
            const unsigned int base = one ? 0u : (unsigned int)a.n1;
            const unsigned int j = one ? (unsigned int)(a.n1 - a.wa + k) : (unsigned int)(a.n2 - a.wb + (k - a.wa));
            const unsigned int t = base + (unsigned int)((hi * (u64)(j + 1u)) >> 32);
            bool seen = false;
#pragma unroll
            for (int q = 0; q < k; ++q) seen |= picks[q] == t;
            picks[k] = seen ? base + j : t;                                        // Floyd's rule
            const unsigned int kappa = 1u + (unsigned int)((lo * (one ? 3ull : 15ull)) >> 32);
            const u64* e = eff + (size_t)(2u * (unsigned int)site_loc[picks[k]]) * LDR;
            if (kappa & 1u) {
#pragma unroll
                for (int w = 0; w < LDR; ++w) out[w] ^= e[w];
            }
            if (kappa & 2u) {
#pragma unroll
                for (int w = 0; w < LDR; ++w) out[w] ^= e[LDR + w];
            }
            if (!one) {                                                            // the target's two effects: location l + 1
                if (kappa & 4u) {
#pragma unroll
                    for (int w = 0; w < LDR; ++w) out[w] ^= e[2 * LDR + w];
                }
                if (kappa & 8u) {
#pragma unroll
                    for (int w = 0; w < LDR; ++w) out[w] ^= e[3 * LDR + w];
                }
                c += (kappa & 3u) != 0u && (kappa >> 2) != 0u ? 1u : 0u;
            }
        }
    }
    return c;
}

template <int LDR, int RULE, bool STAGED = false>
__global__ __launch_bounds__(CIRC_THREADS) void gate_strata_kernel(GateStrataArgs a) {
    constexpr int F = RULE == RULE_EC ? GF2_EC_FIELDS : GF2_FT_FIELDS;
    extern __shared__ u64 gate_strata_lds[];
    u64* eff_lds = gate_strata_lds;
    int* sites_lds = (int*)(eff_lds + (STAGED ? 2 * a.locations * LDR : 0));         // n1 + n2 when staged
    unsigned int* bins = (unsigned int*)(sites_lds + (STAGED ? a.n1 + a.n2 : 0));    // [wb + 1][F]
    const int nbins = (a.wb + 1) * F;
    if (STAGED) {
        for (int i = threadIdx.x; i < 2 * a.locations * LDR; i += blockDim.x) eff_lds[i] = a.eff[i];
        for (int i = threadIdx.x; i < a.n1 + a.n2; i += blockDim.x) sites_lds[i] = a.site_loc[i];
    }
    for (int i = threadIdx.x; i < nbins; i += blockDim.x) bins[i] = 0;
    __syncthreads();
    const u64* eff = STAGED ? eff_lds : a.eff;
    const int* site_loc = STAGED ? sites_lds : a.site_loc;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += stride) {
        const u64 ks = sample_key(a.seed, (u64)(a.first_sample + i));
        u64 out[LDR];
#pragma unroll
        for (int w = 0; w < LDR; ++w) out[w] = 0;
        const unsigned int c = gate_stratum_faults<LDR>(a, eff, site_loc, ks, out);
        const u64 flags = RULE == RULE_EC ? ec_flag_or<LDR>(a, out) : ft_flag_or<LDR>(a, out);
        if (flags) continue;                                                       // a verification fired: the attempt is repeated
        unsigned int* bin = bins + c * F;                                          // c <= wb
        atomicAdd(&bin[0], 1u);
        if constexpr (RULE == RULE_EC) {
            bool flip[2], miss[2];
            unsigned int unmatched[2] = {0, 0};
            ec_chain<LDR>(a, out, flip, miss, unmatched);
            if (flip[0]) atomicAdd(&bin[1], 1u);
            if (flip[1]) atomicAdd(&bin[2], 1u);
            if (flip[0] | flip[1]) atomicAdd(&bin[3], 1u);
            if (miss[0]) atomicAdd(&bin[4], 1u);
            if (miss[1]) atomicAdd(&bin[5], 1u);
            if (unmatched[0]) atomicAdd(&bin[6], unmatched[0]);
            if (unmatched[1]) atomicAdd(&bin[7], unmatched[1]);
        } else {
            unsigned int wrong_trials = 0, first_wrong = 0, unmatched[2] = {0, 0};
            ft_walk<LDR>(a, out, wrong_trials, first_wrong, unmatched);
            if (2 * wrong_trials > (unsigned int)a.trials) atomicAdd(&bin[1], 1u);
            if (wrong_trials) atomicAdd(&bin[2], wrong_trials);
            if (first_wrong) atomicAdd(&bin[3], 1u);
            if (wrong_trials != 0u && wrong_trials != (unsigned int)a.trials) atomicAdd(&bin[4], 1u);
            if (unmatched[0]) atomicAdd(&bin[5], unmatched[0]);
            if (unmatched[1]) atomicAdd(&bin[6], unmatched[1]);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nbins; i += blockDim.x)
        if (bins[i]) atomicAdd(&a.counts[i], (u64)bins[i]);
}

namespace {
struct DevSites {                                                                       // the call's device copy of site_loc
    gf2_ctx* ctx;
    void* dev = nullptr;
    explicit DevSites(gf2_ctx* c) : ctx(c) {}
    ~DevSites() { (void)gf2_dev_free(ctx, dev); }
};
}  // namespace

// The strata of a call whose circuit and layout are checked: tables and site table made once, every stratum cut into launches of
// at most GATE_STRATA_LAUNCH_SAMPLES samples, the counts back once.
template <int RULE>
static int gate_strata(const char* who, gf2_ctx* ctx, const gf2_circuit* circuit, GateStrataArgs& a, const uint64_t* keys1,
                       const uint8_t* flips1, int64_t entries1, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                       const int32_t* site_loc, int64_t n1, int64_t n2, uint64_t seed, int64_t first_sample, int64_t nstrata,
                       const int32_t* wa, const int32_t* wb, const int64_t* counts, uint64_t* counts_out) {
    constexpr int F = RULE == RULE_EC ? GF2_EC_FIELDS : GF2_FT_FIELDS;
    constexpr int64_t PER = (int64_t)GATE_STRATA_ROWS * F;                              // counts per stratum
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    GF2_TRY(gf2_gate_check_sites(who, circuit->locations, site_loc, n1, n2));
    if (nstrata < 0 || nstrata > GF2_STRATA_MAX || (nstrata && (!wa || !wb || !counts)))
        GF2_FAIL(GF2_E_ARG, "%s: needs 0 <= nstrata <= %d and their a, b and counts", who, GF2_STRATA_MAX);
    if (first_sample < 0) GF2_FAIL(GF2_E_ARG, "%s: negative range (needs first_sample >= 0)", who);
    int64_t total = 0;
    for (int64_t s = 0; s < nstrata; ++s) {
        char at[32];
        snprintf(at, sizeof at, "stratum %lld ", (long long)s);
        GF2_TRY(gf2_gate_check_stratum(who, at, n1, n2, wa[s], wb[s]));
        if (counts[s] < 0) GF2_FAIL(GF2_E_ARG, "%s: stratum %lld has a negative sample count (needs counts >= 0)", who, (long long)s);
        total += counts[s] > 0;
    }
    GF2_TRY(gf2_ctx_activate(ctx));
    for (int64_t k = 0; k < PER * nstrata; ++k) counts_out[k] = 0;
    if (total == 0) return GF2_OK;
    CircuitTables tables(ctx);
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, PER * nstrata, &a));
    DevSites sites(ctx);
    GF2_TRY(gf2_dev_alloc(ctx, (size_t)(n1 + n2) * 4, &sites.dev));
    GF2_TRY(gf2_h2d(ctx, sites.dev, site_loc, (size_t)(n1 + n2) * 4));
    a.eff = circuit->eff_dev;
    a.site_loc = (const int*)sites.dev;
    a.locations = (int)circuit->locations;
    a.n1 = (int)n1;
    a.n2 = (int)n2;
    a.seed = seed;
    size_t lds;
    const bool staged = circuit_staged(circuit, RULE == RULE_EC, (size_t)PER * 4, &lds);   // (the measurement's tables never fit)
    if (staged) lds += (size_t)(n1 + n2) * 4;                                            // site_loc beside the effect table
    for (int64_t s = 0; s < nstrata; ++s) {
        a.wa = (int)wa[s];
        a.wb = (int)wb[s];
        a.counts = tables.counts_dev + PER * s;
        for (int64_t done = 0; done < counts[s]; done += GATE_STRATA_LAUNCH_SAMPLES) {
            a.first_sample = first_sample + done;
            a.count = counts[s] - done < GATE_STRATA_LAUNCH_SAMPLES ? counts[s] - done : GATE_STRATA_LAUNCH_SAMPLES;
            int64_t blocks = gf2_cdiv(a.count, CIRC_THREADS * 16);
            if (blocks > GATE_STRATA_MAX_BLOCKS) blocks = GATE_STRATA_MAX_BLOCKS;
            if (blocks < 1) blocks = 1;
            GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
            gadget_for_ldr<RULE>(circuit->ldr, [&](auto ldr) {
                constexpr int LDR = decltype(ldr)::value;
                if constexpr (RULE == RULE_EC) {
                    if (staged) {
                        hipLaunchKernelGGL((gate_strata_kernel<LDR, RULE, true>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
                        return;
                    }
                }
                hipLaunchKernelGGL((gate_strata_kernel<LDR, RULE, false>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
            });
            GF2_TRY(gf2_prof_end(ctx));
            GF2_HIP(hipGetLastError());
        }
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, (size_t)nstrata * PER * 8);
}

extern "C" {

int gf2_mc_ec_decode_gate_strata(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1,
                                 const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                                 int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, uint64_t seed, int64_t first_sample,
                                 int64_t nstrata, const int32_t* a, const int32_t* b, const int64_t* counts, uint64_t* counts_out) {
    const char* who = "gf2_mc_ec_decode_gate_strata";
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GateStrataArgs args = {};
    GF2_TRY(ec_rule_args(who, circuit, rounds, r1, r2, &args));
    return gate_strata<RULE_EC>(who, ctx, circuit, args, keys1, flips1, entries1, keys2, flips2, entries2, site_loc, n1, n2, seed,
                                first_sample, nstrata, a, b, counts, counts_out);
}

int gf2_mc_ft_decode_gate_strata(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                                 const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                                 const uint8_t* flips2, int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, uint64_t seed,
                                 int64_t first_sample, int64_t nstrata, const int32_t* a, const int32_t* b, const int64_t* counts,
                                 uint64_t* counts_out) {
    const char* who = "gf2_mc_ft_decode_gate_strata";
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GateStrataArgs args = {};
    GF2_TRY(ft_rule_args(who, circuit, nsteps, measure_mask, r1, r2, &args));
    return gate_strata<RULE_FT>(who, ctx, circuit, args, keys1, flips1, entries1, keys2, flips2, entries2, site_loc, n1, n2, seed,
                                first_sample, nstrata, a, b, counts, counts_out);
}

}  // extern "C"
