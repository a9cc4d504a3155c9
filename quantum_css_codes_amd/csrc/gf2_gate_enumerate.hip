// Exact strata of the two post-selected gadgets under gate-level faults (include/gf2hip.h "gate-level
// faults"): every configuration of w <= GATE_MAX_W faulty gates of the error-correction cycle or of a rewritten one-qubit program
// -- a = w - b one-operand sites with a kind in {X, Y, Z} each and b CNOT sites with one of the 15 two-qubit Paulis each -- judged
// by the gadget's own tally rule, post-selection included, and counted by the number c of CNOT picks whose kind acts on both
// operands.  Nothing is sampled.
//
// The kernel is gadget_enumerate_kernel's (gf2_gadget_enumerate.hip) with another walk: lane = subset, runs of up to ENUM_MAX_RUN
// consecutive ranks per lane, grid-strided; the flag OR first and the rule skipped for a wavefront with no accepted live lane;
// ballots into the workgroup's LDS bins [c][F] (at most 5 x 8 dwords), sum fields bit by bit; the bins flushed once per workgroup;
// every loop with a workgroup-uniform trip count; out[] and the picks never indexed at run time.
//
// The walk.  rank = r_s + C(n_1, a) r_c: a run unranks the two parts once (enum_unrank_pick of gf2_enumerate_dev.h on four picks
// each) and then steps the product order -- the one-operand part takes its colexicographic successor; when it is at its last
// subset it restarts at 0 .. a - 1 and the CNOT part steps.  After either the lane reads site_loc for its picks (once per subset,
// through L2) and keeps the first locations in VGPRs.  The 3^a 15^b kind assignments are walked in a reflected mixed-radix Gray
// code, the a digits of radix 3 below the b digits of radix 15, the kind mask of digit value v being (v + 1) ^ ((v + 1) >> 1):
// X, Y, Z on a one-operand site and the 4-bit binary-reflected Gray code without 0 on a CNOT.  All radices are odd, so a digit is
// reflected when the number formed by the digits above it is odd, every trip moves one digit by one value and flips one bit of one
// mask: one LDR-word XOR per configuration.  The trip, the moving digit, the bit and c are the same in every lane (scalar
// registers); the moving pick's location is selected on the scalar digit index.
//
// Tallies as in gadget_enumerate_kernel: a configuration adds at most GATE_MAX_ADD to a bin and a launch covers at most
// GATE_LAUNCH_CONFIGS = 2^28 configurations, so a workgroup that walked a whole launch alone keeps every 32-bit bin below 2^32.
#include "gf2_enumerate_dev.h"
#include "gf2_gadget_dev.h"

#define GATE_MAX_W GF2_GATE_ENUMERATE_MAX_WEIGHT
#define GATE_LAUNCH_CONFIGS (1ll << 28)        // configurations per launch: 15 * 2^28 < 2^32
#define GATE_MAX_ADD 15                        // the most one configuration adds to one bin (unmatched keys of 15 steps)
static_assert(GATE_MAX_ADD * GATE_LAUNCH_CONFIGS < (1ll << 32), "a workgroup's 32-bit bins must hold a whole launch");
static_assert(GF2_FT_MAX_LDR - 1 <= GATE_MAX_ADD && GF2_EC_MAX_ROUNDS <= GATE_MAX_ADD, "a sum field's value per configuration");
static_assert(GATE_MAX_W == 4, "the picks are held four and four");

// gf2_host.cpp: the argument rules of a rank range of sites, shared with the host statements
int gf2_gate_check_range(const char* who, int64_t locations, const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b,
                         int64_t first_rank, int64_t count);

struct GateEnumArgs {
    const u64* eff;
    const int* site_loc;                       // n1 + n2 first locations, the one-operand sites first
    int locations, n1, n2;
    int wa, wb;                                // one-operand picks, CNOT picks
    unsigned int nkinds;                       // 3^wa 15^wb
    int run;                                   // consecutive ranks per lane
    u64 c1;                                    // C(n1, wa)
    u64 first_rank;
    int64_t count;                             // subsets of this launch
    int rounds;                                // the cycle
    int nsteps, trials, first_measure;         // the measurement: steps; set bits of measure_mask; its lowest set bit
    unsigned int measure_mask;
    u64 mask[2];                               // [0]: the r_2 bits of key_x, [1]: the r_1 bits of key_z
    int kwx, kwz;                              // 1 and 1 (CircuitTables reads them)
    HashTab tab[2];                            // [0]: parity_check_c2's table (key_x), [1]: parity_check_c1's (key_z)
    const unsigned char* flips[2];             // operator . correction of every table entry
    u64* counts;                               // [(wb + 1)][F]
};

// The k <= 4 picks of the subset of rank r among [0, n), n >= k (the picks from k up are 0): enum_unrank on four picks.
__device__ __forceinline__ void gate_unrank(int k, u64 r, unsigned int n, unsigned int (&pos)[GATE_MAX_W]) {
    unsigned int hi = n;
    pos[3] = k > 3 ? enum_unrank_pick<4>(r, hi) : 0u;
    pos[2] = k > 2 ? enum_unrank_pick<3>(r, hi) : 0u;
    pos[1] = k > 1 ? enum_unrank_pick<2>(r, hi) : 0u;
    pos[0] = k > 0 ? enum_unrank_pick<1>(r, hi) : 0u;
}

// enum_successor on four picks.
__device__ __forceinline__ void gate_successor(int k, unsigned int (&pos)[GATE_MAX_W]) {
    bool done = false;
#pragma unroll
    for (int j = 0; j < GATE_MAX_W; ++j) {
        if (j < k && !done) {
            const bool can = j == k - 1 || pos[j] + 1 < pos[j + 1 < GATE_MAX_W ? j + 1 : j];
            pos[j] = can ? pos[j] + 1 : (unsigned int)j;
            done = can;
        }
    }
}

// The successor of the product order (a live subset is not the last of all: when the one-operand part wraps, the CNOT part can
// step).  Both candidates are computed and selected, so the picks stay in registers; the one not taken is dropped unread.
__device__ __forceinline__ void gate_product_successor(const GateEnumArgs& a, unsigned int (&ps)[GATE_MAX_W], unsigned int (&pc)[GATE_MAX_W]) {
    const bool wrap = a.wa == 0 || ps[0] == (unsigned int)(a.n1 - a.wa);
    unsigned int ns[GATE_MAX_W], nc[GATE_MAX_W];
#pragma unroll
    for (int k = 0; k < GATE_MAX_W; ++k) ns[k] = ps[k], nc[k] = pc[k];
    gate_successor(a.wa, ns);
    gate_successor(a.wb, nc);
#pragma unroll
    for (int k = 0; k < GATE_MAX_W; ++k) {
        ps[k] = wrap ? (k < a.wa ? (unsigned int)k : 0u) : ns[k];
        pc[k] = wrap ? nc[k] : pc[k];
    }
}

// The first locations of the picks (0 for a pick the subset does not have).  ps[k] < n1 and pc[k] < n2 for the picks it has.
__device__ __forceinline__ void gate_locations(const GateEnumArgs& a, const unsigned int (&ps)[GATE_MAX_W], const unsigned int (&pc)[GATE_MAX_W],
                                               unsigned int (&ls)[GATE_MAX_W], unsigned int (&lc)[GATE_MAX_W]) {
#pragma unroll
    for (int k = 0; k < GATE_MAX_W; ++k) {
        ls[k] = k < a.wa ? (unsigned int)a.site_loc[ps[k]] : 0u;
        lc[k] = k < a.wb ? (unsigned int)a.site_loc[(unsigned int)a.n1 + pc[k]] : 0u;
    }
}

__device__ __forceinline__ unsigned int gate_select(const unsigned int (&l)[GATE_MAX_W], int j) {
    const unsigned int l0 = l[0], l1 = l[1], l2 = l[2], l3 = l[3];           // (every pick read first: enum_gray_step's comment)
    unsigned int p = l0;
    p = j == 1 ? l1 : p;
    p = j == 2 ? l2 : p;
    p = j == 3 ? l3 : p;
    return p;
}

__device__ __forceinline__ unsigned int gate_kappa(unsigned int v) { return (v + 1u) ^ ((v + 1u) >> 1); }
__device__ __forceinline__ int gate_two_operand(unsigned int kappa) { return (kappa & 3u) != 0u && (kappa >> 2) != 0u ? 1 : 0; }

// Trip t > 0 of the Gray code (all of it scalar): digit j moves -- among the wa digits of radix 3 or, above them, the wb digits of
// radix 15 -- from value `was` to `now`, one apart; the masks of the two differ in one bit.  Returns the index of the effect whose
// words are XOR-ed in, relative to the moving pick's first location (2 * operand + component); c follows.
__device__ __forceinline__ unsigned int gate_gray_step(unsigned int t, int wa, int& j, int& c) {
    unsigned int q = t, radix = 3u;
    j = 0;
    while (j < wa && q % 3u == 0u) q /= 3u, ++j;
    if (j == wa) {
        radix = 15u;
        while (q % 15u == 0u) q /= 15u, ++j;
    }
    const unsigned int digit = q % radix, above = q / radix;
    const unsigned int now = (above & 1u) ? radix - 1u - digit : digit, was = (above & 1u) ? radix - digit : digit - 1u;
    const unsigned int k_now = gate_kappa(now), k_was = gate_kappa(was);
    if (radix == 15u) c += gate_two_operand(k_now) - gate_two_operand(k_was);
    return (unsigned int)__builtin_ctz(k_now ^ k_was);
}

template <int LDR, int RULE, bool STAGED>
__global__ __launch_bounds__(CIRC_THREADS) void gate_enumerate_kernel(GateEnumArgs a) {
    constexpr int F = RULE == RULE_EC ? GF2_EC_FIELDS : GF2_FT_FIELDS;
    extern __shared__ u64 gate_lds[];
    u64* eff_lds = gate_lds;
    unsigned int* bins = (unsigned int*)(eff_lds + (STAGED ? 2 * a.locations * LDR : 0));
    const int nbins = (a.wb + 1) * F;
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
        // a lane without a run walks rank 0: picks 0 .. a - 1 and 0 .. b - 1, all below n_1 and n_2
        const u64 rank = first < a.count ? a.first_rank + (u64)first : 0ull;
        unsigned int ps[GATE_MAX_W], pc[GATE_MAX_W], ls[GATE_MAX_W], lc[GATE_MAX_W];
        gate_unrank(a.wa, rank % a.c1, (unsigned int)a.n1, ps);
        gate_unrank(a.wb, rank / a.c1, (unsigned int)a.n2, pc);
        for (int step = 0; step < a.run; ++step) {
            const bool live = first + step < a.count;
            if (step > 0 && live) gate_product_successor(a, ps, pc);
            gate_locations(a, ps, pc, ls, lc);
            u64 out[LDR];
#pragma unroll
            for (int q = 0; q < LDR; ++q) out[q] = 0;
#pragma unroll
            for (int k = 0; k < GATE_MAX_W; ++k) {                                     // every mask 1: X, or X on the control
                if (k < a.wa) {
                    const u64* e = eff + (size_t)(2u * ls[k]) * LDR;
#pragma unroll
                    for (int q = 0; q < LDR; ++q) out[q] ^= e[q];
                }
                if (k < a.wb) {
                    const u64* e = eff + (size_t)(2u * lc[k]) * LDR;
#pragma unroll
                    for (int q = 0; q < LDR; ++q) out[q] ^= e[q];
                }
            }
            int c = 0;
            for (unsigned int t = 0; t < a.nkinds; ++t) {
                if (t > 0) {
                    int j;
                    const unsigned int bit = gate_gray_step(t, a.wa, j, c);
                    const unsigned int one = gate_select(ls, j), two = gate_select(lc, j - a.wa);
                    const unsigned int p = j < a.wa ? one : two;
                    const u64* e = eff + (size_t)(2u * p + bit) * LDR;                 // bit = 2 * operand + component
#pragma unroll
                    for (int q = 0; q < LDR; ++q) out[q] ^= e[q];
                }
                const u64 flags = RULE == RULE_EC ? ec_flag_or<LDR>(a, out) : ft_flag_or<LDR>(a, out);
                const bool acc = live && flags == 0ull;
                const u64 accepted = __ballot(acc);
                if (accepted == 0ull) continue;                                        // (wave-uniform) every live lane was rejected
                unsigned int* bin = bins + c * F;
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

namespace {
struct DevSites {                                                                       // the call's device copy of site_loc
    gf2_ctx* ctx;
    void* dev = nullptr;
    explicit DevSites(gf2_ctx* c) : ctx(c) {}
    ~DevSites() { (void)gf2_dev_free(ctx, dev); }
};
}  // namespace

// The launches of a checked call: tables and site table made once, the range cut into launches of at most GATE_LAUNCH_CONFIGS
// configurations.
template <int RULE>
static int gate_enumerate(const char* who, gf2_ctx* ctx, const gf2_circuit* circuit, GateEnumArgs& a, const uint64_t* keys1,
                          const uint8_t* flips1, int64_t entries1, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                          const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank, int64_t count,
                          uint64_t* counts_out) {
    constexpr int F = RULE == RULE_EC ? GF2_EC_FIELDS : GF2_FT_FIELDS;
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    GF2_TRY(gf2_gate_check_range(who, circuit->locations, site_loc, n1, n2, w, b, first_rank, count));
    GF2_TRY(gf2_ctx_activate(ctx));
    const int64_t ncounts = (b + 1) * F;
    for (int64_t k = 0; k < ncounts; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;                                                       // (count > 0: a <= n_1 and b <= n_2)
    CircuitTables tables(ctx);
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, ncounts, &a));
    DevSites sites(ctx);
    GF2_TRY(gf2_dev_alloc(ctx, (size_t)(n1 + n2) * 4, &sites.dev));
    GF2_TRY(gf2_h2d(ctx, sites.dev, site_loc, (size_t)(n1 + n2) * 4));
    a.eff = circuit->eff_dev;
    a.site_loc = (const int*)sites.dev;
    a.locations = (int)circuit->locations;
    a.n1 = (int)n1;
    a.n2 = (int)n2;
    a.wa = (int)(w - b);
    a.wb = (int)b;
    a.nkinds = 1;
    for (int64_t k = 0; k < w; ++k) a.nkinds *= k < w - b ? 3u : 15u;
    unsigned __int128 c1 = 1;                                                            // C(n_1, a) < 2^63 (checked)
    for (int64_t i = 0; i < w - b; ++i) c1 = c1 * (unsigned __int128)(n1 - (w - b) + 1 + i) / (unsigned)(i + 1);
    a.c1 = (u64)c1;
    a.counts = tables.counts_dev;
    size_t lds;
    const bool staged = circuit_staged(circuit, RULE == RULE_EC, (size_t)ncounts * 4, &lds);   // (the measurement's tables never fit)
    const int64_t per_launch = GATE_LAUNCH_CONFIGS / a.nkinds;                           // subsets (at least 2^28 / 15^4)
    if (per_launch < 1 || per_launch * a.nkinds * GATE_MAX_ADD >= (1ll << 32))          // (a workgroup's 32-bit bins: the comment above)
        GF2_FAIL(GF2_E_ARG, "%s: a launch of %lld configurations would overflow a 32-bit bin", who, (long long)(per_launch * a.nkinds));
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
                    hipLaunchKernelGGL((gate_enumerate_kernel<LDR, RULE, true>), dim3(blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
                    return;
                }
            }
            hipLaunchKernelGGL((gate_enumerate_kernel<LDR, RULE, false>), dim3(blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
        });
        GF2_TRY(gf2_prof_end(ctx));
        GF2_HIP(hipGetLastError());
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, (size_t)ncounts * 8);
}

extern "C" {

int gf2_ec_gate_enumerate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                          int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                          const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank, int64_t count,
                          uint64_t* counts_out) {
    const char* who = "gf2_ec_gate_enumerate";
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GateEnumArgs a = {};
    GF2_TRY(ec_rule_args(who, circuit, rounds, r1, r2, &a));
    return gate_enumerate<RULE_EC>(who, ctx, circuit, a, keys1, flips1, entries1, keys2, flips2, entries2, site_loc, n1, n2, w, b, first_rank,
                                   count, counts_out);
}

int gf2_ft_gate_enumerate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1, const uint64_t* keys1,
                          const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                          const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank, int64_t count,
                          uint64_t* counts_out) {
    const char* who = "gf2_ft_gate_enumerate";
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GateEnumArgs a = {};
    GF2_TRY(ft_rule_args(who, circuit, nsteps, measure_mask, r1, r2, &a));
    return gate_enumerate<RULE_FT>(who, ctx, circuit, a, keys1, flips1, entries1, keys2, flips2, entries2, site_loc, n1, n2, w, b, first_rank,
                                   count, counts_out);
}

}  // extern "C"
