// Repeat-until-success Monte-Carlo of the streamed gadgets under gate-level faults (DESIGN.md section 5d "Repeat-until-success under
// gate-level faults", include/gf2hip.h).  gf2_retry.hip's walk with gf2_gate_mc.hip's draw: a retried region -- a preparation with
// its verifications -- is redrawn inside the kernel until its own flag rows are zero, and an attempt draws the region's one-operand
// gates (probability p_1, one of 3 kinds) and then its CNOTs (one event of probability p_2, one of 15 kinds).  Regions are cut at gate
// boundaries, so the sites of a region partition its locations and a region's faults never reach into another region: sites fail
// independently, a flag row depends on one region only, and the accepted samples have the distribution post-selection gives.  With
// max_attempts = 1 this is gate-level post-selection of any length.
//
// Lane = sample, 256 lanes per workgroup, grid-stride.  Blocks and the regions of a block are walked in uniform loops with scalar
// descriptors; the retry loop is the one divergent loop.  One (local, tail, flags) accumulator per lane; inside an attempt the two
// classes are gathered in turn, each in segments of 512 sites with one draw and one inverse-CDF look-up per segment, Floyd's rule
// against the lane's 512-bit taken map in LDS, which serves both classes.  The flags are tested before any lookup.  No array takes a
// run-time index.
//
// Tally: gf2_retry.hip's, word for word (zero_ok included): thirteen 32-bit bins, the attempts in 64 bits at every level.
//
// LDS per workgroup: one inverse-CDF table per distinct (class, segment size), packed to nb + 1 entries; the taken maps; the bins; and
// the block types' tables with the site table when all of that fits RG_LDS_MAX, otherwise both are read through L2.
#include <limits.h>

#include <new>
#include <vector>

#include "gf2_internal.h"
#include "gf2_circuit_dev.h"
#include "gf2_retry_gate_plan.h"
#include "gf2_retry_gate_dev.h"

#define RG_FIELDS GF2_RETRY_FIELDS
#define RG_BINS 13                              // the 32-bit bins: every field but the attempts
#define RG_LDS_MAX (160 * 1024)                 // gf2_stream.hip's budget
#define RG_MAX_BLOCKS 4096
#define RG_FIRST_MEASURE 4                      // bit of RetryGateArgs::info[b].x beside the kind

static_assert(RG_FIELDS == GF2_STREAM_FIELDS + 2, "the streamed fields, exhausted, attempts");
static_assert(GF2_SEG_BITS == 512, "gf2_retry_gate_plan cuts a class into segments of 512 sites");

// gf2_host.cpp: the argument rules of the rates and the range, shared with the host statement
int gf2_gate_check_mc(const char* who, double p1, double p2, int64_t first_sample, int64_t count);

enum { RG_STORE = 0, RG_TALLY = 1 };

struct gf2_retry_gate {
    StreamPlan plan;
    RetryPlan retry;
    RetryGatePlan gate;
    int64_t nblocks, table_words, sites;       // blocks, the FINAL step included; words of all types' tables; sites of all types
    int cdf_words, full_off[2];                // words of the packed inverse-CDF tables; where a class's table of nb = 512 starts
    std::vector<int> cdf_off[2];               // per class: where the table of every distinct size starts
    u64* eff_dev;
    int* site_dev;                             // sites: the row of a site's first location in eff_dev (6 words a row)
    int4* info_dev;                            // nblocks: (kind | RG_FIRST_MEASURE, step or -1, first flag row, 0)
    int2* span_dev;                            // nblocks: the block's regions [first, end) among region_dev
    int4* region_dev;                          // 2 per region of every type: (first site, n_1, n_2, retried), (its last segments' tables, 0, 0)
};

struct RetryGateArgs {
    const u64* eff;
    const int* site;
    int eff_words, sites;
    u64 seed;
    int64_t first_sample, count;
    const u64* cdf;
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
__global__ __launch_bounds__(CIRC_THREADS) void retry_gate_kernel(RetryGateArgs a) {
    extern __shared__ u64 rg_lds[];
    u64* cdf_lds = rg_lds;                                                         // the packed tables of both classes
    u64* eff_lds = rg_lds + a.cdf_words;
    u64* attempts_bin = eff_lds + (STAGED ? a.eff_words : 0);
    int* site_lds = (int*)(attempts_bin + 1);
    unsigned int* taken = (unsigned int*)(site_lds + (STAGED ? a.sites : 0));
    unsigned int* bins = taken + CIRC_THREADS * CIRC_TAKEN_STRIDE;                 // RG_BINS
    for (int i = threadIdx.x; i < a.cdf_words; i += blockDim.x) cdf_lds[i] = a.cdf[i];
    if (STAGED) {
        for (int i = threadIdx.x; i < a.eff_words; i += blockDim.x) eff_lds[i] = a.eff[i];
        for (int i = threadIdx.x; i < a.sites; i += blockDim.x) site_lds[i] = a.site[i];
    }
    if (MODE == RG_TALLY && threadIdx.x < RG_BINS) bins[threadIdx.x] = 0;
    if (MODE == RG_TALLY && threadIdx.x == 0) *attempts_bin = 0;
    __syncthreads();
    const u64* eff = STAGED ? eff_lds : a.eff;
    const int* site = STAGED ? site_lds : a.site;
    unsigned int* mine = taken + threadIdx.x * CIRC_TAKEN_STRIDE;
    unsigned int local[RG_BINS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    u64 all_attempts = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += stride) {
        const u64 ks = sample_key(a.seed, (u64)(a.first_sample + i));
        u64 T = 0, K[2] = {0, 0};                                                  // the data frame; syndrome of the errors recorded so far, per side
        unsigned int P[2] = {0, 0}, unmatched[2] = {0, 0};                         // ... and their operator parity
        unsigned int wrong_trials = 0, first_wrong = 0, final_bits = 0;           // final_bits: flip_x, flip_z, miss_x, miss_z
        u64 attempts = 0;
        u64* row = MODE == RG_STORE ? a.out + i * a.ldo : nullptr;
        if constexpr (MODE == RG_STORE)
            for (int q = 0; q < a.flag_words; ++q) row[a.nsteps + q] = 0;
        bool alive = true;
        u64 g = 0;                                                                 // the region's number in the whole sequence (uniform)
        for (int b = 0; b < a.nblocks; ++b) {
            const int4 info = a.info[b];
            const int2 span = a.span[b];
            u64 bl = 0, bt = 0;                                                    // the block's local and tail words
            for (int r = span.x; r < span.y; ++r, ++g) {
                const int4 reg = a.region[2 * r], tab = a.region[2 * r + 1];
                if (alive) {
                    const u64 kr = segment_draw(ks, GF2_RETRY_SLOT_BASE + g);
                    const int limit = reg.w ? a.max_attempts : 1;
                    u64 l, t, f;
                    int att = 0;
                    do {                                                           // the one divergent loop
                        const u64 ka = mix64(kr + GF2_GOLDEN * (u64)(att + 1));
                        l = t = f = 0;
                        retry_gate_class<false>(reg.y, reg.x, cdf_lds + tab.x, cdf_lds + a.full_off[0], eff, site, mine, ka, l, t, f);
                        retry_gate_class<true>(reg.z, reg.x + reg.y, cdf_lds + tab.y, cdf_lds + a.full_off[1], eff, site, mine, ka, l, t, f);
                        att += 1;
                    } while (f != 0 && att < limit);
                    if (reg.w) attempts += (u64)att;
                    if (f != 0) {                                                  // no attempt passed: the sample is exhausted
                        alive = false;
                        if constexpr (MODE == RG_STORE) {
                            u64* fw = row + a.nsteps + (info.z >> 6);
                            const int sh = info.z & 63;
                            fw[0] |= f << sh;
                            if (sh && (f >> (64 - sh))) fw[1] |= f >> (64 - sh);   // (a bit below the type's flag rows: the word exists)
                        }
                    }
                    bl ^= l, bt ^= t;
                }
            }
            const int kind = info.x & 3;
            const u64 frame = kind == GF2_STREAM_EC ? ~(1ull << 31 | 1ull << 63) : kind == GF2_STREAM_MEASURE ? 0xFFFFFFFFull : kind == GF2_STREAM_FINAL ? ~0ull : 0ull;
            const u64 word = (T & frame) ^ bl;
            if constexpr (MODE == RG_STORE) {
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
                        if (info.x & RG_FIRST_MEASURE) first_wrong = bad;
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
        if constexpr (MODE == RG_STORE) row[a.nsteps + a.flag_words] = attempts;
        if constexpr (MODE == RG_TALLY) {
            all_attempts += attempts;
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
    if constexpr (MODE == RG_TALLY) {
#pragma unroll
        for (int k = 0; k < RG_BINS; ++k)
            if (local[k]) atomicAdd(&bins[k], local[k]);
        if (all_attempts) atomicAdd(attempts_bin, all_attempts);
        __syncthreads();
        if (threadIdx.x < RG_BINS && bins[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (u64)bins[threadIdx.x]);
        if (threadIdx.x == RG_BINS && *attempts_bin) atomicAdd(&a.counts[RG_BINS], *attempts_bin);
    }
}

// gf2_retry.hip's rule: a lane adds at most nsteps to a 32-bit field per sample, a workgroup's 32-bit LDS bins hold the sum over its
// 256 lanes, so with at most `per_lane` samples per lane 256 * per_lane * nsteps must stay below 2^32.  The attempts are 64-bit.
static int64_t rg_per_lane_cap(int64_t nsteps) { return (int64_t)(0xFFFFFFFFll / (256 * (nsteps > 1 ? nsteps : 1))); }
static_assert(0xFFFFFFFFll / (256ll * (GF2_CIRCUIT_MAX_LOCATIONS + 1)) >= 1, "one sample per lane never wraps a 32-bit bin");

namespace {
struct RetryGateBuffer {                                                                // a device buffer of the call's, freed with it
    gf2_ctx* ctx;
    void* dev = nullptr;
    explicit RetryGateBuffer(gf2_ctx* c) : ctx(c) {}
    ~RetryGateBuffer() { (void)gf2_dev_free(ctx, dev); }
};
}  // namespace

// What a launch keeps in LDS besides the block tables and the site table: the packed inverse-CDF tables, the attempts' bin, the
// taken maps and the bins.
static size_t rg_base_lds(size_t cdf_words) { return cdf_words * 8 + 8 + (size_t)CIRC_THREADS * CIRC_TAKEN_STRIDE * 4 + 16 * 4; }
// the full tables of GF2_RETRY_MAX_SIZES sizes of both classes, the taken maps and the bins fit the budget without any block table
static_assert((size_t)2 * GF2_RETRY_MAX_SIZES * GF2_SEG_CDF * 8 + 8 + (size_t)CIRC_THREADS * CIRC_TAKEN_STRIDE * 4 + 16 * 4 <= RG_LDS_MAX, "LDS budget");

template <int MODE>
static int retry_gate_launch(gf2_ctx* ctx, const gf2_retry_gate* rt, const RetryGateArgs& a) {
    const size_t tables = (size_t)rt->table_words * 8 + (size_t)rt->sites * 4;
    const size_t base = rg_base_lds((size_t)rt->cdf_words);
    const bool staged = base + tables <= RG_LDS_MAX;
    const size_t lds = base + (staged ? tables : 0);
    // samples per lane: a long gadget is many segments per sample, so fewer samples per lane keep the grid wide
    int64_t per_lane = 64 / gf2_cdiv(rt->plan.locations, GF2_SEG_BITS);
    if (per_lane > 16) per_lane = 16;
    if (per_lane < 1) per_lane = 1;
    const int64_t cap = rg_per_lane_cap(rt->plan.nsteps);
    if (per_lane > cap) per_lane = cap;
    int64_t blocks = gf2_cdiv(a.count, CIRC_THREADS * per_lane);
    if (blocks > RG_MAX_BLOCKS) blocks = RG_MAX_BLOCKS;                             // (the caller keeps count <= RG_MAX_BLOCKS * 256 * cap)
    if (blocks < 1) blocks = 1;
    if (lds > 64 * 1024) {
        if (staged)
            GF2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(retry_gate_kernel<MODE, true>), hipFuncAttributeMaxDynamicSharedMemorySize, RG_LDS_MAX));
        else
            GF2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(retry_gate_kernel<MODE, false>), hipFuncAttributeMaxDynamicSharedMemorySize, RG_LDS_MAX));
    }
    GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
    if (staged)
        hipLaunchKernelGGL((retry_gate_kernel<MODE, true>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    else
        hipLaunchKernelGGL((retry_gate_kernel<MODE, false>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    GF2_TRY(gf2_prof_end(ctx));
    GF2_HIP(hipGetLastError());
    return GF2_OK;
}

// What a call's kernel arguments take from the handle and the rates, and the call's inverse-CDF tables (made here, uploaded into
// `cdf`, a buffer of the call's).
static int retry_gate_args(const char* who, gf2_ctx* ctx, const gf2_retry_gate* rt, uint64_t seed, double p1, double p2, int64_t max_attempts,
                           RetryGateBuffer* cdf, RetryGateArgs* a) {
    const uint64_t T[2] = {gf2_quantise(p1), gf2_quantise(p2)};
    std::vector<u64> host;
    try {
        host.resize((size_t)(rt->cdf_words > 0 ? rt->cdf_words : 1));
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    for (int c = 0; c < 2; ++c)
        for (size_t k = 0; k < rt->gate.sizes[c].size(); ++k)
            binomial_cdf_table(T[c], rt->gate.sizes[c][k], host.data() + rt->cdf_off[c][k], rt->gate.sizes[c][k] + 1);
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

static int retry_gate_check_attempts(const char* who, int64_t max_attempts) {
    if (max_attempts < 1 || max_attempts > GF2_RETRY_MAX_ATTEMPTS)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= max_attempts <= %d, got %lld", who, GF2_RETRY_MAX_ATTEMPTS, (long long)max_attempts);
    return GF2_OK;
}

extern "C" {

int gf2_retry_gate_destroy(gf2_ctx* ctx, gf2_retry_gate* retry) {
    if (!ctx) GF2_FAIL(GF2_E_ARG, "gf2_retry_gate_destroy: null context");
    if (!retry) return GF2_OK;
    GF2_TRY(gf2_ctx_activate(ctx));
    (void)gf2_dev_free(ctx, retry->eff_dev);
    (void)gf2_dev_free(ctx, retry->site_dev);
    (void)gf2_dev_free(ctx, retry->info_dev);
    (void)gf2_dev_free(ctx, retry->span_dev);
    (void)gf2_dev_free(ctx, retry->region_dev);
    delete retry;
    return GF2_OK;
}

int gf2_retry_gate_create(gf2_ctx* ctx, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                          const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                          const int64_t* type_nregions, const int32_t* site_loc, const int64_t* site_regions, gf2_retry_gate** retry_out) {
    const char* who = "gf2_retry_gate_create";
    if (!ctx || !retry_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    *retry_out = nullptr;
    gf2_retry_gate* rt = new (std::nothrow) gf2_retry_gate();
    if (!rt) GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    rt->eff_dev = nullptr, rt->site_dev = nullptr, rt->info_dev = nullptr, rt->span_dev = nullptr, rt->region_dev = nullptr;
    int rc = gf2_retry_gate_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, nblocks, type_regions, type_nregions,
                                 site_loc, site_regions, 1, &rt->plan, &rt->retry, &rt->gate);
    if (rc != GF2_OK) {
        delete rt;
        return rc;
    }
    const StreamPlan& plan = rt->plan;
    const RetryPlan& retry = rt->retry;
    const RetryGatePlan& gate = rt->gate;
    rt->nblocks = nblocks;
    rt->sites = gate.sites;
    int64_t rows = 0;
    for (int64_t t = 0; t < ntypes; ++t) rows += type_locations[t];
    rt->table_words = rows * 6;
    std::vector<int4> info, region;
    std::vector<int2> span;
    std::vector<int> site;
    try {
        info.resize((size_t)nblocks);
        span.resize((size_t)nblocks);
        region.resize(2 * retry.first.size());
        site.resize((size_t)gate.sites);
        for (int c = 0; c < 2; ++c) rt->cdf_off[c].assign(gate.sizes[c].size(), 0);
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
    rt->cdf_words = words;
    for (int64_t t = 0; t < ntypes; ++t)
        for (int64_t q = retry.type_first[(size_t)t]; q < retry.type_first[(size_t)t + 1]; ++q) {
            const int n1 = gate.n[0][(size_t)q], n2 = gate.n[1][(size_t)q];
            region[2 * (size_t)q] = make_int4((int)gate.site_first[(size_t)q], n1, n2, retry.retried[(size_t)q]);
            region[2 * (size_t)q + 1] = make_int4(n1 > 0 ? rt->cdf_off[0][(size_t)gate.last_size[0][(size_t)q]] : 0,
                                                  n2 > 0 ? rt->cdf_off[1][(size_t)gate.last_size[1][(size_t)q]] : 0, 0, 0);
            for (int64_t s = gate.site_first[(size_t)q]; s < gate.site_first[(size_t)q] + n1 + n2; ++s)
                site[(size_t)s] = (int)(plan.type_offset[(size_t)t] + site_loc[s]);          // the row in the tables of all types
        }
    bool seen_measure = false;
    for (int64_t b = 0; b < nblocks; ++b) {
        const int kind = block_kind[b];
        info[(size_t)b] = make_int4(kind | (kind == GF2_STREAM_MEASURE && !seen_measure ? RG_FIRST_MEASURE : 0), plan.step[(size_t)b], plan.flag[(size_t)b], 0);
        seen_measure |= kind == GF2_STREAM_MEASURE;
        span[(size_t)b] = kind == GF2_STREAM_FINAL ? make_int2(0, 0)
                                                   : make_int2((int)retry.type_first[(size_t)block_type[b]], (int)retry.type_first[(size_t)block_type[b] + 1]);
    }
    rc = gf2_ctx_activate(ctx);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, (size_t)rt->table_words * 8, (void**)&rt->eff_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, site.size() * 4, (void**)&rt->site_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, info.size() * 16, (void**)&rt->info_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, span.size() * 8, (void**)&rt->span_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, region.size() * 16, (void**)&rt->region_dev);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->eff_dev, type_eff, (size_t)rt->table_words * 8);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->site_dev, site.data(), site.size() * 4);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->info_dev, info.data(), info.size() * 16);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->span_dev, span.data(), span.size() * 8);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->region_dev, region.data(), region.size() * 16);
    if (rc != GF2_OK) {
        (void)gf2_retry_gate_destroy(ctx, rt);
        return rc;
    }
    *retry_out = rt;
    return GF2_OK;
}

int gf2_retry_gate_outcomes_dev(gf2_ctx* ctx, const gf2_retry_gate* retry, uint64_t seed, int64_t first_sample, int64_t count, double p1,
                                double p2, int64_t max_attempts, uint64_t* out_dev, int64_t ldo) {
    const char* who = "gf2_retry_gate_outcomes_dev";
    if (!ctx || !retry) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GF2_TRY(retry_gate_check_attempts(who, max_attempts));
    GF2_TRY(gf2_gate_check_mc(who, p1, p2, first_sample, count));
    const int64_t ldr = retry->plan.nsteps + retry->plan.flag_words + 1;
    if (ldo < ldr) GF2_FAIL(GF2_E_ARG, "%s: ldo must be at least the sequence's nsteps + F + 1 = %lld words", who, (long long)ldr);
    if (count == 0) return GF2_OK;
    if (!out_dev) GF2_FAIL(GF2_E_ARG, "%s: null buffer", who);
    GF2_TRY(gf2_ctx_activate(ctx));
    RetryGateArgs a = {};
    RetryGateBuffer cdf(ctx);
    GF2_TRY(retry_gate_args(who, ctx, retry, seed, p1, p2, max_attempts, &cdf, &a));
    a.ldo = ldo;
    const int64_t most = (int64_t)RG_MAX_BLOCKS * CIRC_THREADS * 16;
    for (int64_t done = 0; done < count; done += most) {
        a.first_sample = first_sample + done;
        a.count = count - done < most ? count - done : most;
        a.out = (u64*)out_dev + done * ldo;
        GF2_TRY((retry_gate_launch<RG_STORE>(ctx, retry, a)));
    }
    return gf2_ctx_sync(ctx);                                                      // (the call's tables are freed on return)
}

int gf2_mc_retry_gate_decode(gf2_ctx* ctx, const gf2_retry_gate* retry, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                             int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed,
                             int64_t first_sample, int64_t count, double p1, double p2, int64_t max_attempts, uint64_t* counts_out) {
    const char* who = "gf2_mc_retry_gate_decode";
    if (!ctx || !retry || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GF2_TRY(gf2_stream_check_bits(who, retry->plan, r1, r2));
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    GF2_TRY(retry_gate_check_attempts(who, max_attempts));
    GF2_TRY(gf2_gate_check_mc(who, p1, p2, first_sample, count));
    GF2_TRY(gf2_ctx_activate(ctx));
    for (int k = 0; k < RG_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    RetryGateArgs a = {};
    RetryGateBuffer cdf(ctx);
    GF2_TRY(retry_gate_args(who, ctx, retry, seed, p1, p2, max_attempts, &cdf, &a));
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
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, RG_FIELDS, &a));
    a.counts = tables.counts_dev;
    const int64_t most = (int64_t)RG_MAX_BLOCKS * CIRC_THREADS * rg_per_lane_cap(retry->plan.nsteps);
    for (int64_t done = 0; done < count; done += most) {
        a.first_sample = first_sample + done;
        a.count = count - done < most ? count - done : most;
        GF2_TRY((retry_gate_launch<RG_TALLY>(ctx, retry, a)));
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, RG_FIELDS * 8);              // (waits for the launches: the call's tables are freed on return)
}

}  // extern "C"
