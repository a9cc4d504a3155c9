// Exact strata of the two post-selected gadgets (DESIGN.md "Exact strata of the cycle", "Exact strata of the measurement"): every
// fault configuration of weight w <= ENUM_MAX_W of the error-correction cycle or of a rewritten one-qubit program -- a subset S of
// the L locations with a kind in {X, Y, Z} per pick -- judged by the gadget's own tally rule, post-selection included, and counted
// per kind composition (n_x, n_y).  Nothing is sampled.
//
// The walk is enumerate_kernel's (gf2_enumerate_dev.h): lane = subset, runs of up to ENUM_MAX_RUN consecutive ranks per lane, one
// unranking per run and the colexicographic successor after it, the 3^w kind assignments in the reflected ternary Gray code with
// one LDR-word XOR per configuration; t, j and the composition in scalar registers, the eight picks in VGPRs, every loop with a
// workgroup-uniform trip count (lanes without a subset walk along with `live` off).  The rule is the samplers' (gf2_gadget_dev.h):
// the chain of ec_kernel or the step walk of ft_kernel on the lane's outcome words.
//
// Post-selection: most configurations are rejected (a verification sees the fault), so the flag OR comes first and a wavefront in
// which no live lane is accepted skips the rule altogether -- a ballot, wave-uniform, no barrier inside the loop.  Rejected lanes of
// a wavefront that does walk look up keys of their own (any key is a valid probe) and are masked out of every ballot.
//
// Tallies: the composition is wave-uniform, so a field's count over the wavefront is the population count of a ballot, added by one
// lane to the workgroup's LDS bins [n_x][n_y][F] (at most 81 x 8 dwords) only when it is non-zero; the fields that are sums and not
// indicators (trial_wrong <= 7, unmatched_x / unmatched_z <= 15, round_unmatched_* <= 6) are added bit by bit as
// sum_b 2^b popcount(ballot(bit b)).  The bins go to global memory once per workgroup.  A configuration adds at most 15 to a bin and
// a launch covers at most GADGET_LAUNCH_CONFIGS = 2^28 configurations, so even a workgroup that walked a whole launch alone keeps
// every 32-bit bin below 15 * 2^28 < 2^32 (checked where the launches are cut).
#include "gf2_enumerate_dev.h"
#include "gf2_gadget_dev.h"

#define GADGET_LAUNCH_CONFIGS (1ll << 28)      // configurations per launch: 15 * 2^28 < 2^32 (the comment above)
#define GADGET_MAX_ADD 15                      // the most one configuration adds to one bin (unmatched keys of 15 steps)
static_assert(GADGET_MAX_ADD * GADGET_LAUNCH_CONFIGS < (1ll << 32), "a workgroup's 32-bit bins must hold a whole launch");
static_assert(GF2_FT_MAX_LDR - 1 <= GADGET_MAX_ADD && GF2_EC_MAX_ROUNDS <= GADGET_MAX_ADD, "a sum field's value per configuration");

struct GadgetEnumArgs {
    const u64* eff;
    int locations, weight;
    unsigned int pow3;                         // 3^weight
    int run;                                   // consecutive ranks per lane
    u64 first_rank;
    int64_t count;                             // subsets of this launch
    int rounds;                                // the cycle
    int nsteps, trials, first_measure;         // the measurement: steps; set bits of measure_mask; its lowest set bit
    unsigned int measure_mask;
    u64 mask[2];                               // [0]: the r_2 bits of key_x, [1]: the r_1 bits of key_z
    int kwx, kwz;                              // 1 and 1 (CircuitTables reads them)
    HashTab tab[2];                            // [0]: parity_check_c2's table (key_x), [1]: parity_check_c1's (key_z)
    const unsigned char* flips[2];             // operator . correction of every table entry
    u64* counts;                               // [(weight + 1)][(weight + 1)][F]
};

template <int LDR, int RULE, bool STAGED>
__global__ __launch_bounds__(CIRC_THREADS) void gadget_enumerate_kernel(GadgetEnumArgs a) {
    constexpr int F = RULE == RULE_EC ? GF2_EC_FIELDS : GF2_FT_FIELDS;
    extern __shared__ u64 gadget_lds[];
    u64* eff_lds = gadget_lds;
    unsigned int* bins = (unsigned int*)(eff_lds + (STAGED ? 2 * a.locations * LDR : 0));
    const int w = a.weight, side = w + 1, nbins = side * side * F;
    if (STAGED)
        for (int i = threadIdx.x; i < 2 * a.locations * LDR; i += blockDim.x) eff_lds[i] = a.eff[i];
    for (int i = threadIdx.x; i < nbins; i += blockDim.x) bins[i] = 0;
    __syncthreads();
    const u64* eff = STAGED ? eff_lds : a.eff;
    const bool first_lane = (threadIdx.x & 63) == 0;
    const int64_t nruns = (a.count + a.run - 1) / a.run;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < nruns; base += stride) {
        const int64_t run = base + threadIdx.x;
        const int64_t first = run * a.run;                                             // of this lane, within the launch
        unsigned int pos[ENUM_MAX_W];
        // a lane without a run unranks rank 0: picks 0 .. w - 1, all below L
        enum_unrank(w, first < a.count ? a.first_rank + (u64)first : 0ull, (unsigned int)a.locations, pos);
        for (int step = 0; step < a.run; ++step) {
            const bool live = first + step < a.count;
            if (step > 0 && live) enum_successor(w, pos);
            u64 out[LDR];
            enum_all_x<LDR>(w, eff, pos, out);                                         // all X
            int n_x = w, n_y = 0;
            for (unsigned int t = 0; t < a.pow3; ++t) {
                if (t > 0) {
                    bool xy;
                    const unsigned int p = enum_gray_step(t, pos, xy, n_x, n_y);
                    const u64* e = eff + (size_t)(2 * p + (xy ? 1u : 0u)) * LDR;
#pragma unroll
                    for (int q = 0; q < LDR; ++q) out[q] ^= e[q];
                }
                const u64 flags = RULE == RULE_EC ? ec_flag_or<LDR>(a, out) : ft_flag_or<LDR>(a, out);
                const bool acc = live && flags == 0ull;
                const u64 accepted = __ballot(acc);
                if (accepted == 0ull) continue;                                        // (wave-uniform) every live lane was rejected
                unsigned int* bin = bins + (n_x * side + n_y) * F;
                if (first_lane) atomicAdd(&bin[0], (unsigned int)__popcll(accepted));
                if constexpr (RULE == RULE_EC) {
                    bool flip[2], miss[2];
                    unsigned int unmatched[2] = {0, 0};
                    ec_chain<LDR>(a, out, flip, miss, unmatched);
                    ec_add_tally(bin, first_lane, acc, flip, miss, unmatched);
                } else {
                    unsigned int wrong_trials = 0, first_wrong = 0, unmatched[2] = {0, 0};
                    ft_walk<LDR>(a, out, wrong_trials, first_wrong, unmatched);
                    ft_add_tally(bin, first_lane, acc, wrong_trials, first_wrong, unmatched, (unsigned int)a.trials);
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nbins; i += blockDim.x)
        if (bins[i]) atomicAdd(&a.counts[i], (u64)bins[i]);
}

// The launches of a checked call: tables made once, the range cut into launches of at most GADGET_LAUNCH_CONFIGS configurations.
template <int RULE>
static int gadget_enumerate(const char* who, gf2_ctx* ctx, const gf2_circuit* circuit, GadgetEnumArgs& a, const uint64_t* keys1,
                            const uint8_t* flips1, int64_t entries1, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, int64_t w,
                            int64_t first_rank, int64_t count, uint64_t* counts_out) {
    constexpr int F = RULE == RULE_EC ? GF2_EC_FIELDS : GF2_FT_FIELDS;
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    GF2_TRY(gf2_enum_check_range(who, circuit->locations, w, first_rank, count));
    GF2_TRY(gf2_ctx_activate(ctx));
    const int64_t ncounts = (w + 1) * (w + 1) * F;
    for (int64_t k = 0; k < ncounts; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    CircuitTables tables(ctx);
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, ncounts, &a));
    a.eff = circuit->eff_dev;
    a.locations = (int)circuit->locations;
    a.weight = (int)w;
    a.pow3 = 1;
    for (int64_t k = 0; k < w; ++k) a.pow3 *= 3u;
    a.counts = tables.counts_dev;
    size_t lds;
    const bool staged = circuit_staged(circuit, RULE == RULE_EC, (size_t)ncounts * 4, &lds);   // (the measurement's tables never fit)
    const int64_t per_launch = GADGET_LAUNCH_CONFIGS / a.pow3;                           // subsets (at least 2^28 / 3^8)
    if (per_launch < 1 || per_launch * a.pow3 * GADGET_MAX_ADD >= (1ll << 32))          // (a workgroup's 32-bit bins: the comment above)
        GF2_FAIL(GF2_E_ARG, "%s: a launch of %lld configurations would overflow a 32-bit bin", who, (long long)(per_launch * a.pow3));
    for (int64_t done = 0; done < count; done += per_launch) {
        a.first_rank = (u64)(first_rank + done);
        a.count = count - done < per_launch ? count - done : per_launch;
        unsigned blocks;
        enum_launch_shape(a.count, &a.run, &blocks);
        GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
        gadget_for_ldr<RULE>(circuit->ldr, [&](auto ldr) {
            constexpr int LDR = decltype(ldr)::value;
            if constexpr (RULE == RULE_EC) {
                if (staged) {
                    hipLaunchKernelGGL((gadget_enumerate_kernel<LDR, RULE, true>), dim3(blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
                    return;
                }
            }
            hipLaunchKernelGGL((gadget_enumerate_kernel<LDR, RULE, false>), dim3(blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
        });
        GF2_TRY(gf2_prof_end(ctx));
        GF2_HIP(hipGetLastError());
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, (size_t)ncounts * 8);
}

extern "C" {

int gf2_ec_enumerate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                     int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, int64_t w,
                     int64_t first_rank, int64_t count, uint64_t* counts_out) {
    const char* who = "gf2_ec_enumerate";
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GadgetEnumArgs a = {};
    GF2_TRY(ec_rule_args(who, circuit, rounds, r1, r2, &a));
    return gadget_enumerate<RULE_EC>(who, ctx, circuit, a, keys1, flips1, entries1, keys2, flips2, entries2, w, first_rank, count, counts_out);
}

int gf2_ft_enumerate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1, const uint64_t* keys1,
                     const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                     int64_t w, int64_t first_rank, int64_t count, uint64_t* counts_out) {
    const char* who = "gf2_ft_enumerate";
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GadgetEnumArgs a = {};
    GF2_TRY(ft_rule_args(who, circuit, nsteps, measure_mask, r1, r2, &a));
    return gadget_enumerate<RULE_FT>(who, ctx, circuit, a, keys1, flips1, entries1, keys2, flips2, entries2, w, first_rank, count, counts_out);
}

}  // extern "C"
