// Repeat-until-success Monte-Carlo under gate-level faults with waiting faults on the data block (DESIGN.md section 5d
// "Repeat-until-success with waiting faults under gate-level faults", include/gf2hip.h).  gf2_retry_gate.hip's walk and draw plus
// gf2_retry_wait.hip's wait draw: a retried region is redrawn until its own flag rows are zero, an attempt draws the region's
// one-operand gates (p_1, one of 3 kinds) and then its CNOTs (p_2, one of 15 kinds), and every attempt made, the failed ones
// included, also draws the region's wait rows -- the qubits of the data block that wait while the region is prepared -- with the
// memory rates (q_x, q_y, q_z).
//
// retry_gate_kernel's structure stands: lane = sample, 256 lanes per workgroup, grid-stride, uniform block and region loops with
// scalar descriptors, one divergent attempt loop.  Inside that loop, after the two classes, comes the wait draw (gf2_retry_wait_dev.h):
// one error_count under the wait key of (region, attempt), usually K = 0, into a second pair of accumulators per lane (wait local,
// wait tail) that no attempt clears and that are folded into the block's words when the region ends.  The lane's taken map serves
// all three draws.  The wait key is computed only for a region that has wait rows, a uniform condition.  The wait key and the
// region's key are separate streams, so the attempts of every preparation are those gf2_retry_gate.hip makes.  No array takes a
// run-time index.
//
// Tally: retry_gate_kernel's, plus the wait faults drawn over all attempts, 64-bit per lane, per workgroup and per call as the
// attempts are.
//
// LDS per workgroup, in this order: the packed inverse-CDF tables of both classes and of the wait sizes (made per call from p_1, p_2
// and q); the taken maps, the 32-bit bins and two 64-bit bins; the wait rows (4 words per row) when they fit after those, otherwise
// they are read through L2; the block types' tables with the site table when all of that still fits RGW_LDS_MAX, otherwise both are
// read through L2.
#include <limits.h>

#include <new>
#include <vector>

#include "gf2_internal.h"
#include "gf2_circuit_dev.h"
#include "gf2_retry_gate_wait_plan.h"
#include "gf2_retry_gate_dev.h"
#include "gf2_retry_wait_dev.h"

#define RGW_FIELDS GF2_RETRY_WAIT_FIELDS
#define RGW_BINS 13                             // the 32-bit bins: every field but the attempts and the wait faults
#define RGW_LDS_MAX (160 * 1024)                // gf2_retry_gate.hip's budget
#define RGW_MAX_BLOCKS 4096
#define RGW_FIRST_MEASURE 4                     // bit of RetryGateWaitArgs::info[b].x beside the kind

static_assert(RGW_FIELDS == GF2_RETRY_FIELDS + 1 && GF2_RETRY_FIELDS == RGW_BINS + 1, "the retried fields, then the wait faults");
static_assert(GF2_SEG_BITS == 512 && GF2_RETRY_WAIT_MAX_ROWS == GF2_SEG_BITS, "a class is cut into segments of 512 sites; a region's wait rows are one");

// gf2_host.cpp: the argument rules of the rates and the range, shared with the host statement
int gf2_gate_check_mc(const char* who, double p1, double p2, int64_t first_sample, int64_t count);

enum { RGW_STORE = 0, RGW_TALLY = 1 };

struct gf2_retry_gate_wait {
    StreamPlan plan;
    RetryPlan retry;
    RetryGatePlan gate;
    RetryWaitPlan wait;
    int64_t nblocks, table_words, sites, wait_words;  // blocks, the FINAL step included; words of all types' tables; sites of all types; words of all wait rows
    int cdf_words, full_off[2];                // words of the packed inverse-CDF tables, the wait sizes' included; where a class's table of nb = 512 starts
    std::vector<int> cdf_off[2], wcdf_off;     // per class, and of the wait sizes: where the table of every distinct size starts
    u64* eff_dev;
    u64* wait_dev;                             // the wait rows (at least one word)
    int* site_dev;                             // sites: the row of a site's first location in eff_dev (6 words a row)
    int4* info_dev;                            // nblocks: (kind | RGW_FIRST_MEASURE, step or -1, first flag row, 0)
    int2* span_dev;                            // nblocks: the block's regions [first, end) among region_dev
    int4* region_dev;                          // 3 per region of every type: (first site, n_1, n_2, retried), (its last segments' tables, 0, 0),
                                               // (first wait row, wait rows, their table, 0)
};

struct RetryGateWaitArgs {
    const u64* eff;
    const u64* wait_eff;
    const int* site;
    int eff_words, sites, wait_words, wait_lds;   // wait_lds: the wait rows are staged
    u64 seed;
    int64_t first_sample, count;
    u64 w_1, w_2;                              // the kinds' thresholds of q
    const u64* cdf;                            // the tables of p_1, of p_2, then those of q
    int cdf_words, full_off[2];
    const int4* info;
    const int2* span;
    const int4* region;
    int nblocks, nsteps, flag_words, max_attempts;
    // store
    u64* out;
    int64_t ldo;
    // tally
    int trials;
    u64 mask[2];                               // [0]: the r_2 bits of key_x, [1]: the r_1 bits of key_z
    int kwx, kwz;                              // 1 and 1 (CircuitTables reads them)
    HashTab tab[2];                            // [0]: parity_check_c2's table (key_x), [1]: parity_check_c1's (key_z)
    const unsigned char* flips[2];             // operator . correction of every table entry
    int zero_ok[2];                            // the side's table holds the key 0 with flip 0
    u64* counts;
};

template <int MODE, bool STAGED>
__global__ __launch_bounds__(CIRC_THREADS) void retry_gate_wait_kernel(RetryGateWaitArgs a) {
    extern __shared__ u64 rgw_lds[];
    u64* cdf_lds = rgw_lds;                                                        // the packed tables of both classes, then of the wait sizes
    unsigned int* taken = (unsigned int*)(cdf_lds + a.cdf_words);
    unsigned int* bins = taken + CIRC_THREADS * CIRC_TAKEN_STRIDE;                 // RGW_BINS of 16
    u64* wide_bins = (u64*)(bins + 16);                                            // [0]: attempts, [1]: wait faults
    u64* weff_lds = wide_bins + 2;
    u64* eff_lds = weff_lds + (a.wait_lds ? a.wait_words : 0);
    int* site_lds = (int*)(eff_lds + (STAGED ? a.eff_words : 0));
    for (int i = threadIdx.x; i < a.cdf_words; i += blockDim.x) cdf_lds[i] = a.cdf[i];
    if (a.wait_lds)
        for (int i = threadIdx.x; i < a.wait_words; i += blockDim.x) weff_lds[i] = a.wait_eff[i];
    if (STAGED) {
        for (int i = threadIdx.x; i < a.eff_words; i += blockDim.x) eff_lds[i] = a.eff[i];
        for (int i = threadIdx.x; i < a.sites; i += blockDim.x) site_lds[i] = a.site[i];
    }
    if (MODE == RGW_TALLY && threadIdx.x < RGW_BINS) bins[threadIdx.x] = 0;
    if (MODE == RGW_TALLY && threadIdx.x < 2) wide_bins[threadIdx.x] = 0;
    __syncthreads();
    const u64* eff = STAGED ? eff_lds : a.eff;
    const int* site = STAGED ? site_lds : a.site;
    unsigned int* mine = taken + threadIdx.x * CIRC_TAKEN_STRIDE;
    unsigned int local[RGW_BINS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    u64 all_attempts = 0, all_waited = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += stride) {
        const u64 ks = sample_key(a.seed, (u64)(a.first_sample + i));
        u64 T = 0, K[2] = {0, 0};                                                  // the data frame; syndrome of the errors recorded so far, per side
        unsigned int P[2] = {0, 0}, unmatched[2] = {0, 0};                         // ... and their operator parity
        unsigned int wrong_trials = 0, first_wrong = 0, final_bits = 0;           // final_bits: flip_x, flip_z, miss_x, miss_z
        u64 attempts = 0, waited = 0;
        u64* row = MODE == RGW_STORE ? a.out + i * a.ldo : nullptr;
        if constexpr (MODE == RGW_STORE)
            for (int q = 0; q < a.flag_words; ++q) row[a.nsteps + q] = 0;
        bool alive = true;
        u64 g = 0;                                                                 // the region's number in the whole sequence (uniform)
        for (int b = 0; b < a.nblocks; ++b) {
            const int4 info = a.info[b];
            const int2 span = a.span[b];
            u64 bl = 0, bt = 0;                                                    // the block's local and tail words
            for (int r = span.x; r < span.y; ++r, ++g) {
                const int4 reg = a.region[3 * r], tab = a.region[3 * r + 1], wreg = a.region[3 * r + 2];
                if (alive) {
                    const u64 kr = segment_draw(ks, GF2_RETRY_SLOT_BASE + g);
                    const u64 kw = wreg.y > 0 ? segment_draw(ks, GF2_RETRY_WAIT_SLOT_BASE + g) : 0ull;   // (uniform: only a region that has wait rows pays)
                    const int limit = reg.w ? a.max_attempts : 1;
                    u64 l, t, f, wl = 0, wt = 0;                                   // wl, wt: what the data picked up while it waited, never cleared
                    int att = 0;
                    do {                                                           // the one divergent loop
                        const u64 ka = mix64(kr + GF2_GOLDEN * (u64)(att + 1));
                        l = t = f = 0;
                        retry_gate_class<false>(reg.y, reg.x, cdf_lds + tab.x, cdf_lds + a.full_off[0], eff, site, mine, ka, l, t, f);
                        retry_gate_class<true>(reg.z, reg.x + reg.y, cdf_lds + tab.y, cdf_lds + a.full_off[1], eff, site, mine, ka, l, t, f);
                        if (wreg.y > 0) {                                          // the data waits through this attempt, passed or not
                            if (a.wait_lds)
                                waited += (u64)retry_wait_draw<true>(kw, att, wreg.y, cdf_lds + wreg.z, a.w_1, a.w_2, weff_lds + (size_t)wreg.x * 4, mine, wl, wt);
                            else
                                waited += (u64)retry_wait_draw<false>(kw, att, wreg.y, cdf_lds + wreg.z, a.w_1, a.w_2, a.wait_eff + (size_t)wreg.x * 4, mine, wl, wt);
                        }
                        att += 1;
                    } while (f != 0 && att < limit);
                    if (reg.w) attempts += (u64)att;
                    if (f != 0) {                                                  // no attempt passed: the sample is exhausted
                        alive = false;
                        if constexpr (MODE == RGW_STORE) {
                            u64* fw = row + a.nsteps + (info.z >> 6);
                            const int sh = info.z & 63;
                            fw[0] |= f << sh;
                            if (sh && (f >> (64 - sh))) fw[1] |= f >> (64 - sh);   // (a bit below the type's flag rows: the word exists)
                        }
                    }
                    bl ^= l ^ wl, bt ^= t ^ wt;
                }
            }
            const int kind = info.x & 3;
            const u64 frame = kind == GF2_STREAM_EC ? ~(1ull << 31 | 1ull << 63) : kind == GF2_STREAM_MEASURE ? 0xFFFFFFFFull : kind == GF2_STREAM_FINAL ? ~0ull : 0ull;
            const u64 word = (T & frame) ^ bl;
            if constexpr (MODE == RGW_STORE) {
                if (info.y >= 0) row[info.y] = alive ? word : 0ull;
                T ^= bt;
            } else if (alive) {
                if (kind == GF2_STREAM_EC || kind == GF2_STREAM_MEASURE) {
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        if (c == 0 || kind == GF2_STREAM_EC) {                     // a measurement corrects data.x_errors only
                            const u64 v = ((word >> (32 * c)) & a.mask[c]) ^ K[c];
                            if (v != 0 || !a.zero_ok[c]) {                         // (v = 0 and zero_ok: found, K ^= 0, P ^= 0)
                                const u64 hit = hash_find<1>(a.tab[c], 0ull, v);
                                if (hit == ~0ull) {
                                    unmatched[c] += 1;                             // no match, nothing recorded
                                } else {
                                    K[c] ^= v;
                                    P[c] ^= a.flips[c][a.tab[c].val[hit]] & 1u;
                                }
                            }
                        }
                    }
                    if (kind == GF2_STREAM_MEASURE) {
                        const unsigned int bad = (unsigned int)((word >> 31) & 1ull) ^ P[0];
                        wrong_trials += bad;
                        if (info.x & RGW_FIRST_MEASURE) first_wrong = bad;
                    }
                } else if (kind == GF2_STREAM_FINAL) {
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const u64 v = ((word >> (32 * c)) & a.mask[c]) ^ K[c];
                        unsigned int flip = (unsigned int)((word >> (32 * c + 31)) & 1ull) ^ P[c], miss = 0;
                        if (v != 0 || !a.zero_ok[c]) {
                            const u64 hit = hash_find<1>(a.tab[c], 0ull, v);
                            if (hit == ~0ull)
                                miss = 1;
                            else
                                flip ^= a.flips[c][a.tab[c].val[hit]] & 1u;
                        }
                        final_bits |= flip << c | miss << (2 + c);
                    }
                }
                T ^= bt;
            }
        }
        if constexpr (MODE == RGW_STORE) {
            row[a.nsteps + a.flag_words] = attempts;
            row[a.nsteps + a.flag_words + 1] = waited;
        }
        if constexpr (MODE == RGW_TALLY) {
            all_attempts += attempts;
            all_waited += waited;
            if (alive) {
                const unsigned int fx = final_bits & 1u, fz = (final_bits >> 1) & 1u;
                local[0] += 1;
                local[1] += fx;
                local[2] += fz;
                local[3] += fx | fz;
                local[4] += (final_bits >> 2) & 1u;
                local[5] += (final_bits >> 3) & 1u;
                local[6] += unmatched[0];
                local[7] += unmatched[1];
                local[8] += 2 * wrong_trials > (unsigned int)a.trials;
                local[9] += wrong_trials;
                local[10] += first_wrong;
                local[11] += wrong_trials != 0 && wrong_trials != (unsigned int)a.trials;
            } else {
                local[12] += 1;
            }
        }
    }
    if constexpr (MODE == RGW_TALLY) {
#pragma unroll
        for (int k = 0; k < RGW_BINS; ++k)
            if (local[k]) atomicAdd(&bins[k], local[k]);
        if (all_attempts) atomicAdd(&wide_bins[0], all_attempts);
        if (all_waited) atomicAdd(&wide_bins[1], all_waited);
        __syncthreads();
        if (threadIdx.x < RGW_BINS && bins[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (u64)bins[threadIdx.x]);
        if (threadIdx.x >= RGW_BINS && threadIdx.x < RGW_FIELDS && wide_bins[threadIdx.x - RGW_BINS])
            atomicAdd(&a.counts[threadIdx.x], wide_bins[threadIdx.x - RGW_BINS]);
    }
}

// gf2_retry.hip's rule: with at most `per_lane` samples per lane, 256 * per_lane * nsteps must stay below 2^32 for the 32-bit bins.
// The attempts and the wait faults are 64-bit throughout and need no such bound.
static int64_t rgw_per_lane_cap(int64_t nsteps) { return (int64_t)(0xFFFFFFFFll / (256 * (nsteps > 1 ? nsteps : 1))); }

namespace {
struct RetryGateWaitBuffer {                                                            // a device buffer of the call's, freed with it
    gf2_ctx* ctx;
    void* dev = nullptr;
    explicit RetryGateWaitBuffer(gf2_ctx* c) : ctx(c) {}
    ~RetryGateWaitBuffer() { (void)gf2_dev_free(ctx, dev); }
};
}  // namespace

// What a launch keeps in LDS besides the wait rows, the block tables and the site table: the packed inverse-CDF tables, the taken
// maps, the 32-bit bins and the two wide bins.
#define RGW_LDS_FIXED ((size_t)CIRC_THREADS * CIRC_TAKEN_STRIDE * 4 + 16 * 4 + 2 * 8)
static size_t rgw_lds_base(const gf2_retry_gate_wait* rt) { return (size_t)rt->cdf_words * 8 + RGW_LDS_FIXED; }
static bool rgw_wait_staged(const gf2_retry_gate_wait* rt) { return rgw_lds_base(rt) + (size_t)rt->wait_words * 8 <= RGW_LDS_MAX; }
// The worst case of the tables alone -- GF2_RETRY_MAX_SIZES full tables of either class and GF2_RETRY_GATE_WAIT_MAX_SIZES full wait
// tables -- fits the budget with no wait row and no block table staged, and one wait table more would not: the cap is the largest.
static_assert((size_t)(2 * GF2_RETRY_MAX_SIZES + GF2_RETRY_GATE_WAIT_MAX_SIZES) * GF2_SEG_CDF * 8 + RGW_LDS_FIXED <= RGW_LDS_MAX, "LDS budget");
static_assert((size_t)(2 * GF2_RETRY_MAX_SIZES + GF2_RETRY_GATE_WAIT_MAX_SIZES + 1) * GF2_SEG_CDF * 8 + RGW_LDS_FIXED > RGW_LDS_MAX,
              "GF2_RETRY_GATE_WAIT_MAX_SIZES is the largest cap the budget allows");

template <int MODE>
static int retry_gate_wait_launch(gf2_ctx* ctx, const gf2_retry_gate_wait* rt, const RetryGateWaitArgs& a) {
    const size_t tables = (size_t)rt->table_words * 8 + (size_t)rt->sites * 4;
    const size_t base = rgw_lds_base(rt) + (a.wait_lds ? (size_t)rt->wait_words * 8 : 0);
    const bool staged = base + tables <= RGW_LDS_MAX;
    const size_t lds = base + (staged ? tables : 0);
    // samples per lane: a long gadget is many segments per sample, so fewer samples per lane keep the grid wide
    int64_t per_lane = 64 / gf2_cdiv(rt->plan.locations, GF2_SEG_BITS);
    if (per_lane > 16) per_lane = 16;
    if (per_lane < 1) per_lane = 1;
    const int64_t cap = rgw_per_lane_cap(rt->plan.nsteps);
    if (per_lane > cap) per_lane = cap;
    int64_t blocks = gf2_cdiv(a.count, CIRC_THREADS * per_lane);
    if (blocks > RGW_MAX_BLOCKS) blocks = RGW_MAX_BLOCKS;                           // (the caller keeps count <= RGW_MAX_BLOCKS * 256 * cap)
    if (blocks < 1) blocks = 1;
    if (lds > 64 * 1024) {
        if (staged)
            GF2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(retry_gate_wait_kernel<MODE, true>), hipFuncAttributeMaxDynamicSharedMemorySize, RGW_LDS_MAX));
        else
            GF2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(retry_gate_wait_kernel<MODE, false>), hipFuncAttributeMaxDynamicSharedMemorySize, RGW_LDS_MAX));
    }
    GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
    if (staged)
        hipLaunchKernelGGL((retry_gate_wait_kernel<MODE, true>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    else
        hipLaunchKernelGGL((retry_gate_wait_kernel<MODE, false>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    GF2_TRY(gf2_prof_end(ctx));
    GF2_HIP(hipGetLastError());
    return GF2_OK;
}

// What a call's kernel arguments take from the handle and the rates, and the call's inverse-CDF tables of p_1, p_2 and q (made here,
// uploaded into `cdf`, a buffer of the call's).
static int retry_gate_wait_args(const char* who, gf2_ctx* ctx, const gf2_retry_gate_wait* rt, uint64_t seed, double p1, double p2, double q_x,
                                double q_y, double q_z, int64_t max_attempts, RetryGateWaitBuffer* cdf, RetryGateWaitArgs* a) {
    const uint64_t T[2] = {gf2_quantise(p1), gf2_quantise(p2)};
    const double q_t = q_x + q_y + q_z;
    const uint64_t w_any = gf2_quantise(q_t);
    a->w_1 = q_t > 0.0 ? gf2_quantise(q_x / q_t) : 0;
    a->w_2 = q_t > 0.0 ? gf2_quantise((q_x + q_y) / q_t) : 0;
    std::vector<u64> host;
    try {
        host.resize((size_t)(rt->cdf_words > 0 ? rt->cdf_words : 1));
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    for (int c = 0; c < 2; ++c)
        for (size_t k = 0; k < rt->gate.sizes[c].size(); ++k)
            binomial_cdf_table(T[c], rt->gate.sizes[c][k], host.data() + rt->cdf_off[c][k], rt->gate.sizes[c][k] + 1);
    for (size_t k = 0; k < rt->wait.sizes.size(); ++k)
        binomial_cdf_table(w_any, rt->wait.sizes[k], host.data() + rt->wcdf_off[k], rt->wait.sizes[k] + 1);
    GF2_TRY(gf2_dev_alloc(ctx, host.size() * 8, &cdf->dev));
    GF2_TRY(gf2_h2d(ctx, cdf->dev, host.data(), host.size() * 8));
    a->cdf = (const u64*)cdf->dev;
    a->cdf_words = rt->cdf_words;
    a->full_off[0] = rt->full_off[0];
    a->full_off[1] = rt->full_off[1];
    a->eff = rt->eff_dev;
    a->site = rt->site_dev;
    a->eff_words = (int)rt->table_words;
    a->sites = (int)rt->sites;
    a->wait_eff = rt->wait_dev;
    a->wait_words = (int)rt->wait_words;
    a->wait_lds = rgw_wait_staged(rt) ? 1 : 0;
    a->seed = seed;
    a->info = rt->info_dev;
    a->span = rt->span_dev;
    a->region = rt->region_dev;
    a->nblocks = (int)rt->nblocks;
    a->nsteps = (int)rt->plan.nsteps;
    a->flag_words = (int)rt->plan.flag_words;
    a->max_attempts = (int)max_attempts;
    a->trials = (int)rt->plan.trials;
    return GF2_OK;
}

static int retry_gate_wait_check_call(const char* who, int64_t max_attempts, double p1, double p2, double q_x, double q_y, double q_z,
                                      int64_t first_sample, int64_t count) {
    if (max_attempts < 1 || max_attempts > GF2_RETRY_MAX_ATTEMPTS)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= max_attempts <= %d, got %lld", who, GF2_RETRY_MAX_ATTEMPTS, (long long)max_attempts);
    GF2_TRY(gf2_gate_check_mc(who, p1, p2, first_sample, count));
    return gf2_retry_wait_check_rates(who, q_x, q_y, q_z);
}

extern "C" {

int gf2_retry_gate_wait_destroy(gf2_ctx* ctx, gf2_retry_gate_wait* retry) {
    if (!ctx) GF2_FAIL(GF2_E_ARG, "gf2_retry_gate_wait_destroy: null context");
    if (!retry) return GF2_OK;
    GF2_TRY(gf2_ctx_activate(ctx));
    (void)gf2_dev_free(ctx, retry->eff_dev);
    (void)gf2_dev_free(ctx, retry->wait_dev);
    (void)gf2_dev_free(ctx, retry->site_dev);
    (void)gf2_dev_free(ctx, retry->info_dev);
    (void)gf2_dev_free(ctx, retry->span_dev);
    (void)gf2_dev_free(ctx, retry->region_dev);
    delete retry;
    return GF2_OK;
}

int gf2_retry_gate_wait_create(gf2_ctx* ctx, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                               const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                               const int64_t* type_nregions, const int32_t* site_loc, const int64_t* site_regions, const uint64_t* wait_eff,
                               const int64_t* wait_count, gf2_retry_gate_wait** retry_out) {
    const char* who = "gf2_retry_gate_wait_create";
    if (!ctx || !retry_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    *retry_out = nullptr;
    gf2_retry_gate_wait* rt = new (std::nothrow) gf2_retry_gate_wait();
    if (!rt) GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    rt->eff_dev = rt->wait_dev = nullptr, rt->site_dev = nullptr, rt->info_dev = nullptr, rt->span_dev = nullptr, rt->region_dev = nullptr;
    int rc = gf2_retry_gate_wait_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, nblocks, type_regions, type_nregions,
                                      site_loc, site_regions, wait_eff, wait_count, 1, &rt->plan, &rt->retry, &rt->gate, &rt->wait);
    if (rc != GF2_OK) {
        delete rt;
        return rc;
    }
    const StreamPlan& plan = rt->plan;
    const RetryPlan& retry = rt->retry;
    const RetryGatePlan& gate = rt->gate;
    const RetryWaitPlan& wait = rt->wait;
    rt->nblocks = nblocks;
    rt->sites = gate.sites;
    int64_t rows = 0;
    for (int64_t t = 0; t < ntypes; ++t) rows += type_locations[t];
    rt->table_words = rows * 6;
    rt->wait_words = wait.rows * 4;
    std::vector<int4> info, region;
    std::vector<int2> span;
    std::vector<int> site;
    try {
        info.resize((size_t)nblocks);
        span.resize((size_t)nblocks);
        region.resize(3 * retry.first.size());
        site.resize((size_t)gate.sites);
        for (int c = 0; c < 2; ++c) rt->cdf_off[c].assign(gate.sizes[c].size(), 0);
        rt->wcdf_off.assign(wait.sizes.size(), 0);
    } catch (const std::bad_alloc&) {
        delete rt;
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    int words = 0;
    for (int c = 0; c < 2; ++c) {
        for (size_t k = 0; k < gate.sizes[c].size(); ++k) {
            rt->cdf_off[c][k] = words;
            words += gate.sizes[c][k] + 1;
        }
        rt->full_off[c] = gate.full_size[c] >= 0 ? rt->cdf_off[c][(size_t)gate.full_size[c]] : 0;
    }
    for (size_t k = 0; k < wait.sizes.size(); ++k) {                                // the wait sizes' tables follow the classes'
        rt->wcdf_off[k] = words;
        words += wait.sizes[k] + 1;
    }
    rt->cdf_words = words;
    for (int64_t t = 0; t < ntypes; ++t)
        for (int64_t q = retry.type_first[(size_t)t]; q < retry.type_first[(size_t)t + 1]; ++q) {
            const int n1 = gate.n[0][(size_t)q], n2 = gate.n[1][(size_t)q], w = wait.count[(size_t)q];
            region[3 * (size_t)q] = make_int4((int)gate.site_first[(size_t)q], n1, n2, retry.retried[(size_t)q]);
            region[3 * (size_t)q + 1] = make_int4(n1 > 0 ? rt->cdf_off[0][(size_t)gate.last_size[0][(size_t)q]] : 0,
                                                  n2 > 0 ? rt->cdf_off[1][(size_t)gate.last_size[1][(size_t)q]] : 0, 0, 0);
            region[3 * (size_t)q + 2] = make_int4((int)wait.first[(size_t)q], w, w > 0 ? rt->wcdf_off[(size_t)wait.size[(size_t)q]] : 0, 0);
            for (int64_t s = gate.site_first[(size_t)q]; s < gate.site_first[(size_t)q] + n1 + n2; ++s)
                site[(size_t)s] = (int)(plan.type_offset[(size_t)t] + site_loc[s]);          // the row in the tables of all types
        }
    bool seen_measure = false;
    for (int64_t b = 0; b < nblocks; ++b) {
        const int kind = block_kind[b];
        info[(size_t)b] = make_int4(kind | (kind == GF2_STREAM_MEASURE && !seen_measure ? RGW_FIRST_MEASURE : 0), plan.step[(size_t)b], plan.flag[(size_t)b], 0);
        seen_measure |= kind == GF2_STREAM_MEASURE;
        span[(size_t)b] = kind == GF2_STREAM_FINAL ? make_int2(0, 0)
                                                   : make_int2((int)retry.type_first[(size_t)block_type[b]], (int)retry.type_first[(size_t)block_type[b] + 1]);
    }
    const size_t wait_bytes = (size_t)(rt->wait_words > 0 ? rt->wait_words : 1) * 8;
    rc = gf2_ctx_activate(ctx);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, (size_t)rt->table_words * 8, (void**)&rt->eff_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, wait_bytes, (void**)&rt->wait_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, site.size() * 4, (void**)&rt->site_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, info.size() * 16, (void**)&rt->info_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, span.size() * 8, (void**)&rt->span_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, region.size() * 16, (void**)&rt->region_dev);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->eff_dev, type_eff, (size_t)rt->table_words * 8);
    if (rc == GF2_OK && rt->wait_words > 0) rc = gf2_h2d(ctx, rt->wait_dev, wait_eff, (size_t)rt->wait_words * 8);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->site_dev, site.data(), site.size() * 4);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->info_dev, info.data(), info.size() * 16);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->span_dev, span.data(), span.size() * 8);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->region_dev, region.data(), region.size() * 16);
    if (rc != GF2_OK) {
        (void)gf2_retry_gate_wait_destroy(ctx, rt);
        return rc;
    }
    *retry_out = rt;
    return GF2_OK;
}

int gf2_retry_gate_wait_outcomes_dev(gf2_ctx* ctx, const gf2_retry_gate_wait* retry, uint64_t seed, int64_t first_sample, int64_t count,
                                     double p1, double p2, double q_x, double q_y, double q_z, int64_t max_attempts, uint64_t* out_dev,
                                     int64_t ldo) {
    const char* who = "gf2_retry_gate_wait_outcomes_dev";
    if (!ctx || !retry) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GF2_TRY(retry_gate_wait_check_call(who, max_attempts, p1, p2, q_x, q_y, q_z, first_sample, count));
    const int64_t ldr = retry->plan.nsteps + retry->plan.flag_words + 2;
    if (ldo < ldr) GF2_FAIL(GF2_E_ARG, "%s: ldo must be at least the sequence's nsteps + F + 2 = %lld words", who, (long long)ldr);
    if (count == 0) return GF2_OK;
    if (!out_dev) GF2_FAIL(GF2_E_ARG, "%s: null buffer", who);
    GF2_TRY(gf2_ctx_activate(ctx));
    RetryGateWaitArgs a = {};
    RetryGateWaitBuffer cdf(ctx);
    GF2_TRY(retry_gate_wait_args(who, ctx, retry, seed, p1, p2, q_x, q_y, q_z, max_attempts, &cdf, &a));
    a.ldo = ldo;
    const int64_t most = (int64_t)RGW_MAX_BLOCKS * CIRC_THREADS * 16;
    for (int64_t done = 0; done < count; done += most) {
        a.first_sample = first_sample + done;
        a.count = count - done < most ? count - done : most;
        a.out = (u64*)out_dev + done * ldo;
        GF2_TRY((retry_gate_wait_launch<RGW_STORE>(ctx, retry, a)));
    }
    return gf2_ctx_sync(ctx);                                                      // (the call's tables are freed on return)
}

int gf2_mc_retry_gate_wait_decode(gf2_ctx* ctx, const gf2_retry_gate_wait* retry, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                                  int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed,
                                  int64_t first_sample, int64_t count, double p1, double p2, double q_x, double q_y, double q_z,
                                  int64_t max_attempts, uint64_t* counts_out) {
    const char* who = "gf2_mc_retry_gate_wait_decode";
    if (!ctx || !retry || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GF2_TRY(gf2_stream_check_bits(who, retry->plan, r1, r2));                       // (the plan holds the wait rows' bits too)
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    GF2_TRY(retry_gate_wait_check_call(who, max_attempts, p1, p2, q_x, q_y, q_z, first_sample, count));
    GF2_TRY(gf2_ctx_activate(ctx));
    for (int k = 0; k < RGW_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    RetryGateWaitArgs a = {};
    RetryGateWaitBuffer cdf(ctx);
    GF2_TRY(retry_gate_wait_args(who, ctx, retry, seed, p1, p2, q_x, q_y, q_z, max_attempts, &cdf, &a));
    a.mask[0] = (1ull << r2) - 1;
    a.mask[1] = (1ull << r1) - 1;
    a.kwx = a.kwz = 1;
    const uint64_t* ks[2] = {keys2, keys1};
    const uint8_t* fs[2] = {flips2, flips1};
    const int64_t es[2] = {entries2, entries1};
    for (int c = 0; c < 2; ++c)                                                    // the fast path's premise, checked here: key 0 -> flip 0
        for (int64_t e = 0; e < es[c]; ++e)
            if (ks[c][e] == 0 && (fs[c][e] & 1) == 0) a.zero_ok[c] = 1;
    CircuitTables tables(ctx);
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, RGW_FIELDS, &a));
    a.counts = tables.counts_dev;
    const int64_t most = (int64_t)RGW_MAX_BLOCKS * CIRC_THREADS * rgw_per_lane_cap(retry->plan.nsteps);
    for (int64_t done = 0; done < count; done += most) {
        a.first_sample = first_sample + done;
        a.count = count - done < most ? count - done : most;
        a.out = nullptr;
        GF2_TRY((retry_gate_wait_launch<RGW_TALLY>(ctx, retry, a)));
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, RGW_FIELDS * 8);             // (waits for the launches: the call's tables are freed on return)
}

}  // extern "C"
