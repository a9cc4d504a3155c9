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

enum { RULE_EC = 0, RULE_FT = 1 };

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

__device__ __forceinline__ void gate_add_votes(unsigned int* bin, bool first_lane, bool vote) {
    const u64 votes = __ballot(vote);
    if (votes != 0ull && first_lane) atomicAdd(bin, (unsigned int)__popcll(votes));
}

template <int BITS>
__device__ __forceinline__ void gate_add_sum(unsigned int* bin, bool first_lane, bool acc, unsigned int value) {
    unsigned int sum = 0;
#pragma unroll
    for (int b = 0; b < BITS; ++b) sum += (unsigned int)__popcll(__ballot(acc && ((value >> b) & 1u))) << b;
    if (sum != 0u && first_lane) atomicAdd(bin, sum);
}

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
                    gate_add_votes(&bin[1], first_lane, acc && flip[0]);
                    gate_add_votes(&bin[2], first_lane, acc && flip[1]);
                    gate_add_votes(&bin[3], first_lane, acc && (flip[0] || flip[1]));
                    gate_add_votes(&bin[4], first_lane, acc && miss[0]);
                    gate_add_votes(&bin[5], first_lane, acc && miss[1]);
                    gate_add_sum<3>(&bin[6], first_lane, acc, unmatched[0]);           // <= GF2_EC_MAX_ROUNDS = 6
                    gate_add_sum<3>(&bin[7], first_lane, acc, unmatched[1]);
                } else {
                    unsigned int wrong_trials = 0, first_wrong = 0, unmatched[2] = {0, 0};
                    ft_walk<LDR>(a, out, wrong_trials, first_wrong, unmatched);
                    gate_add_votes(&bin[1], first_lane, acc && 2 * wrong_trials > (unsigned int)a.trials);
                    gate_add_sum<4>(&bin[2], first_lane, acc, wrong_trials);           // <= trials <= 15 steps
                    gate_add_votes(&bin[3], first_lane, acc && first_wrong != 0u);
                    gate_add_votes(&bin[4], first_lane, acc && wrong_trials != 0u && wrong_trials != (unsigned int)a.trials);
                    gate_add_sum<4>(&bin[5], first_lane, acc, unmatched[0]);           // <= nsteps <= 15
                    gate_add_sum<4>(&bin[6], first_lane, acc, unmatched[1]);
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nbins; i += blockDim.x)
        if (bins[i]) atomicAdd(&a.counts[i], (u64)bins[i]);
}

template <int LDR, int RULE>
static void gate_launch_ldr(gf2_ctx* ctx, const GateEnumArgs& a, bool staged, unsigned blocks, size_t lds) {
    if constexpr (RULE == RULE_EC) {
        if (staged) {
            hipLaunchKernelGGL((gate_enumerate_kernel<LDR, RULE, true>), dim3(blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
            return;
        }
    }
    hipLaunchKernelGGL((gate_enumerate_kernel<LDR, RULE, false>), dim3(blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
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
    const size_t eff_bytes = (size_t)2 * circuit->locations * circuit->ldr * 8;
    const bool staged = RULE == RULE_EC && eff_bytes <= CIRC_EFF_LDS_BYTES;             // (the measurement's tables never fit)
    const size_t lds = (staged ? eff_bytes : 0) + (size_t)ncounts * 4;
    const int64_t per_launch = GATE_LAUNCH_CONFIGS / a.nkinds;                           // subsets (at least 2^28 / 15^4)
    if (per_launch < 1 || per_launch * a.nkinds * GATE_MAX_ADD >= (1ll << 32))          // (a workgroup's 32-bit bins: the comment above)
        GF2_FAIL(GF2_E_ARG, "%s: a launch of %lld configurations would overflow a 32-bit bin", who, (long long)(per_launch * a.nkinds));
    for (int64_t done = 0; done < count; done += per_launch) {
        a.first_rank = (u64)(first_rank + done);
        a.count = count - done < per_launch ? count - done : per_launch;
        int64_t run = a.count / ((int64_t)ENUM_MAX_BLOCKS * CIRC_THREADS);               // short runs until every lane has one
        a.run = (int)(run < 1 ? 1 : run > ENUM_MAX_RUN ? ENUM_MAX_RUN : run);
        int64_t blocks = gf2_cdiv(gf2_cdiv(a.count, a.run), CIRC_THREADS);
        if (blocks > ENUM_MAX_BLOCKS) blocks = ENUM_MAX_BLOCKS;
        GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
#define GATE_CASE(L) \
    case L: gate_launch_ldr<L, RULE>(ctx, a, staged, (unsigned)blocks, lds); break;
        if constexpr (RULE == RULE_EC) {
            switch (circuit->ldr) { GATE_CASE(3) GATE_CASE(4) GATE_CASE(5) GATE_CASE(6) GATE_CASE(7) GATE_CASE(8) }
        } else {
            switch (circuit->ldr) {
                GATE_CASE(8) GATE_CASE(9) GATE_CASE(10) GATE_CASE(11) GATE_CASE(12) GATE_CASE(13) GATE_CASE(14) GATE_CASE(15)
                GATE_CASE(16)
            }
        }
#undef GATE_CASE
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
    if (r1 < 1 || r2 < 1 || r1 > 31 || r2 > 31)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= r_1, r_2 <= 31 (the keys share a word), got %lld and %lld", who, (long long)r1, (long long)r2);
    if (rounds < 1 || rounds > GF2_EC_MAX_ROUNDS) GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= rounds <= %d, got %lld", who, GF2_EC_MAX_ROUNDS, (long long)rounds);
    if (circuit->ldr > GF2_CIRCUIT_MAX_LDR)
        GF2_FAIL(GF2_E_ARG, "%s: needs ldr <= %d words per effect, got %lld", who, GF2_CIRCUIT_MAX_LDR, (long long)circuit->ldr);
    if (circuit->ldr < rounds + 2)
        GF2_FAIL(GF2_E_ARG, "%s: %lld rounds need ldr = 1 + rounds + F words with F >= 1 flag words, the circuit has %lld", who,
                 (long long)rounds, (long long)circuit->ldr);
    GateEnumArgs a = {};
    a.rounds = (int)rounds;
    a.mask[0] = (1ull << r2) - 1;
    a.mask[1] = (1ull << r1) - 1;
    a.kwx = a.kwz = 1;
    const u64 keys = a.mask[0] | a.mask[1] << 32;
    bool beyond = (circuit->any[0] & ~(keys | 1ull << 31 | 1ull << 63)) != 0;
    for (int64_t t = 1; t <= rounds; ++t) beyond |= (circuit->any[t] & ~keys) != 0;
    if (beyond) GF2_FAIL(GF2_E_ARG, "%s: the effects set bits beyond the keys' r_2 / r_1 bits, the two parity bits and the flag words", who);
    return gate_enumerate<RULE_EC>(who, ctx, circuit, a, keys1, flips1, entries1, keys2, flips2, entries2, site_loc, n1, n2, w, b, first_rank,
                                   count, counts_out);
}

int gf2_ft_gate_enumerate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1, const uint64_t* keys1,
                          const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                          const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank, int64_t count,
                          uint64_t* counts_out) {
    const char* who = "gf2_ft_gate_enumerate";
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (r1 < 1 || r2 < 1 || r1 > 31 || r2 > 31)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= r_1, r_2 <= 31 (the keys share a word), got %lld and %lld", who, (long long)r1, (long long)r2);
    if (circuit->ldr < 8 || circuit->ldr > GF2_FT_MAX_LDR)
        GF2_FAIL(GF2_E_ARG, "%s: needs 8 <= ldr <= %d words per effect, got %lld", who, GF2_FT_MAX_LDR, (long long)circuit->ldr);
    if (nsteps < 1 || circuit->ldr < nsteps + 1)
        GF2_FAIL(GF2_E_ARG, "%s: needs nsteps >= 1 and ldr = nsteps + F words with F >= 1 flag words, got nsteps = %lld, the circuit has %lld", who,
                 (long long)nsteps, (long long)circuit->ldr);
    if (measure_mask >> nsteps) GF2_FAIL(GF2_E_ARG, "%s: measure_mask has bits at or above nsteps = %lld", who, (long long)nsteps);
    const int trials = __builtin_popcountll(measure_mask);
    if (trials % 2 == 0) GF2_FAIL(GF2_E_ARG, "%s: a majority vote needs an odd number of trials, measure_mask has %d", who, trials);
    GateEnumArgs a = {};
    a.nsteps = (int)nsteps;
    a.trials = trials;
    a.first_measure = __builtin_ctzll(measure_mask);
    a.measure_mask = (unsigned int)measure_mask;
    a.mask[0] = (1ull << r2) - 1;
    a.mask[1] = (1ull << r1) - 1;
    a.kwx = a.kwz = 1;
    bool beyond = false;
    for (int64_t s = 0; s < nsteps; ++s)
        beyond |= (circuit->any[s] & ~((measure_mask >> s) & 1ull ? a.mask[0] | 1ull << 31 : a.mask[0] | a.mask[1] << 32)) != 0;
    if (beyond)
        GF2_FAIL(GF2_E_ARG, "%s: the effects set bits beyond the layout (an EC step's r_2 / r_1 key bits, a MEASURE step's r_2 key bits and bit 31)", who);
    return gate_enumerate<RULE_FT>(who, ctx, circuit, a, keys1, flips1, entries1, keys2, flips2, entries2, site_loc, n1, n2, w, b, first_rank,
                                   count, counts_out);
}

}  // extern "C"
