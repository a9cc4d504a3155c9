// Repeat-until-success Monte-Carlo of multi-block programs under gate-level faults (DESIGN.md section 5d "Repeat-until-success of
// multi-block programs under gate-level faults", include/gf2hip.h): gf2_mretry.hip's walk, frames, records and tally with
// gf2_retry_gate.hip's draw.  Every retried region of a rewritten program on several logical qubits is redrawn, inside the kernel,
// until its own flag rows are zero, and an attempt draws the region's one-operand gates (probability p_1, one of 3 kinds) and then
// its CNOTs (one event of probability p_2, one of 15 kinds).  A CNOT block is one region of n CNOT sites that is never retried: site
// i is the physical CNOT D_a[i] -> D_b[i], its rows hold (tail for a, tail for b, 0), and one event puts a correlated Pauli on both
// frames.  Sites fail independently, no site straddles two regions and a CNOT block has no flag row, so the accepted samples have the
// distribution post-selection gives; max_attempts = 1 is gate-level post-selection of a multi-qubit program.
//
// Lane = sample, 256 lanes per workgroup, grid-stride.  The walk is mretry_kernel's: uniform loops over the blocks and over a
// block's regions with scalar descriptors, one (l, t, f) accumulator per lane, the retry loop as the one divergent loop, the flags
// tested before any lookup.  The draw inside an attempt is retry_gate_class<false> then <true> (gf2_retry_gate_dev.h), with
// retry_gate_kernel's region descriptors.  The frames and records are mretry_kernel's: T[NF] and the packed record R[NF], picked and
// put back through chains of selects over compile-time indices.  Instantiated on NF in {1, 2, 4} (three frames run as four); no
// scratch, no array takes a run-time index (DESIGN.md has the build's figures).
//
// Tally: mretry_kernel's, word for word: `accepted` and the attempts in registers, the rare fields to the workgroup's twenty-one
// 32-bit LDS bins, the attempts in one 64-bit bin.
//
// LDS per workgroup: one inverse-CDF table per distinct (class, segment size), packed to nb + 1 entries; the 512-bit taken maps;
// the bins; and the block types' tables with the site table when all of that fits MG_LDS_MAX, otherwise both are read through L2.
#include <limits.h>

#include <new>
#include <vector>

#include "gf2_internal.h"
#include "gf2_circuit_dev.h"
#include "gf2_mretry_gate_plan.h"
#include "gf2_retry_gate_dev.h"

#define MG_FIELDS GF2_MRETRY_FIELDS
#define MG_BINS 21                              // the 32-bit bins: every field but the attempts
#define MG_EXHAUSTED GF2_MSTREAM_FIELDS         // the bin, and the field, of the exhausted samples
#define MG_LDS_MAX (160 * 1024)                 // gf2_stream.hip's budget
#define MG_MAX_BLOCKS 4096
#define MG_LOW 0x00000000FFFFFFFFull
#define MG_HIGH 0xFFFFFFFF00000000ull

static_assert(MG_FIELDS == GF2_MSTREAM_FIELDS + 2 && MG_BINS == GF2_MSTREAM_FIELDS + 1, "the multi-block fields, exhausted, attempts");
static_assert(GF2_SEG_BITS == 512, "gf2_retry_gate_site_rules cuts a class into segments of 512 sites");

// gf2_host.cpp: the argument rules of the rates and the range, shared with the host statement
int gf2_gate_check_mc(const char* who, double p1, double p2, int64_t first_sample, int64_t count);

enum { MG_STORE = 0, MG_TALLY = 1 };

struct gf2_mretry_gate {
    MStreamPlan plan;
    RetryPlan retry;
    RetryGatePlan gate;
    int64_t nblocks, table_words, sites;       // blocks; words of all types' tables; sites of all types
    int cdf_words, full_off[2];                // words of the packed inverse-CDF tables; where a class's table of nb = 512 starts
    std::vector<int> cdf_off[2];               // per class: where the table of every distinct size starts
    u64* eff_dev;
    int* site_dev;                             // sites: the row of a site's first location in eff_dev (6 words a row)
    int4* info_dev;                            // nblocks: (kind | first trial << 3 | a << 4 | b << 6 | measurement << 8, step or -1, first flag row, 0)
    int2* span_dev;                            // nblocks: the block's regions [first, end) among region_dev
    int4* region_dev;                          // 2 per region of every type: (first site, n_1, n_2, retried), (its last segments' tables, 0, 0)
};

struct MRetryGateArgs {
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
    int trials, measurements, propagated;
    u64 mask[2];                               // [0]: the r_2 bits of key_x, [1]: the r_1 bits of key_z
    int kwx, kwz;                              // 1 and 1 (CircuitTables reads them)
    HashTab tab[2];                            // [0]: parity_check_c2's table (key_x), [1]: parity_check_c1's (key_z)
    const unsigned char* flips[2];             // operator . correction of every table entry
    int zero_ok[2];                            // the side's table holds the key 0 with flip 0
    u64* counts;
};

template <int MODE, bool STAGED, int NF>
__global__ __launch_bounds__(CIRC_THREADS) void mretry_gate_kernel(MRetryGateArgs a) {
    extern __shared__ u64 mg_lds[];
    u64* cdf_lds = mg_lds;                                                         // the packed tables of both classes
    u64* eff_lds = mg_lds + a.cdf_words;
    u64* attempts_bin = eff_lds + (STAGED ? a.eff_words : 0);
    int* site_lds = (int*)(attempts_bin + 1);
    unsigned int* taken = (unsigned int*)(site_lds + (STAGED ? a.sites : 0));
    unsigned int* bins = taken + CIRC_THREADS * CIRC_TAKEN_STRIDE;                 // MG_BINS
    for (int i = threadIdx.x; i < a.cdf_words; i += blockDim.x) cdf_lds[i] = a.cdf[i];
    if (STAGED) {
        for (int i = threadIdx.x; i < a.eff_words; i += blockDim.x) eff_lds[i] = a.eff[i];
        for (int i = threadIdx.x; i < a.sites; i += blockDim.x) site_lds[i] = a.site[i];
    }
    if (MODE == MG_TALLY && threadIdx.x < MG_BINS) bins[threadIdx.x] = 0;
    if (MODE == MG_TALLY && threadIdx.x == 0) *attempts_bin = 0;
    __syncthreads();
    const u64* eff = STAGED ? eff_lds : a.eff;
    const int* site = STAGED ? site_lds : a.site;
    unsigned int* mine = taken + threadIdx.x * CIRC_TAKEN_STRIDE;
    unsigned int accepted = 0;
    u64 all_attempts = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += stride) {
        const u64 ks = sample_key(a.seed, (u64)(a.first_sample + i));
        u64 T[NF], R[NF];                                                          // the data frames; the records, packed as a frame is
#pragma unroll
        for (int q = 0; q < NF; ++q) T[q] = R[q] = 0;
        unsigned int unmatched[2] = {0, 0};
        unsigned int wrong_trials = 0, first_wrong = 0;                            // a byte per measurement; a bit per measurement
        u64 attempts = 0;
        u64* row = MODE == MG_STORE ? a.out + i * a.ldo : nullptr;
        if constexpr (MODE == MG_STORE)
            for (int q = 0; q < a.flag_words; ++q) row[a.nsteps + q] = 0;
        bool alive = true;
        u64 g = 0;                                                                 // the region's number in the whole sequence (uniform)
        for (int b = 0; b < a.nblocks; ++b) {
            const int4 info = a.info[b];
            const int2 span = a.span[b];
            u64 bl = 0, bt = 0;                                                    // local and tail; a CNOT block's: tail for a, tail for b
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
                        if constexpr (MODE == MG_STORE) {
                            u64* fw = row + a.nsteps + (info.z >> 6);
                            const int sh = info.z & 63;
                            fw[0] |= f << sh;
                            if (sh && (f >> (64 - sh))) fw[1] |= f >> (64 - sh);   // (a bit below the type's flag rows: the word exists)
                        }
                    }
                    bl ^= l, bt ^= t;
                }
            }
            // close the block (all of it uniform but the lanes' own words)
            const int kind = info.x & 7, fa = (info.x >> 4) & 3, fb = (info.x >> 6) & 3;
            u64 Ta = 0, Tb = 0;
#pragma unroll
            for (int q = 0; q < NF; ++q) {
                if (q == fa) Ta = T[q];
                if (q == fb) Tb = T[q];
            }
            if (kind == GF2_MSTREAM_CNOT) {                                        // (fa != fb; no word, no flags: `alive` is unchanged)
                if (alive) {
                    Tb ^= Ta & MG_LOW;
                    Ta ^= Tb & MG_HIGH;
                    Ta ^= bl, Tb ^= bt;
#pragma unroll
                    for (int q = 0; q < NF; ++q) {
                        if (q == fa) T[q] = Ta;
                        if (q == fb) T[q] = Tb;
                    }
                    if constexpr (MODE == MG_TALLY) {
                        if (a.propagated) {
                            u64 Ra = 0, Rb = 0;
#pragma unroll
                            for (int q = 0; q < NF; ++q) {
                                if (q == fa) Ra = R[q];
                                if (q == fb) Rb = R[q];
                            }
                            Rb ^= Ra & MG_LOW;
                            Ra ^= Rb & MG_HIGH;
#pragma unroll
                            for (int q = 0; q < NF; ++q) {
                                if (q == fa) R[q] = Ra;
                                if (q == fb) R[q] = Rb;
                            }
                        }
                    }
                }
            } else {
                const u64 frame = kind == GF2_STREAM_EC ? ~(1ull << 31 | 1ull << 63) : kind == GF2_STREAM_MEASURE ? MG_LOW : 0ull;
                const u64 word = (Ta & frame) ^ bl;
                if constexpr (MODE == MG_STORE) {
                    if (info.y >= 0) row[info.y] = alive ? word : 0ull;
                } else if (alive && kind != GF2_STREAM_NONE) {
                    u64 Ra = 0;
#pragma unroll
                    for (int q = 0; q < NF; ++q)
                        if (q == fa) Ra = R[q];
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        if (c == 0 || kind == GF2_STREAM_EC) {                     // a measurement corrects data.x_errors only
                            const u64 v = ((word ^ Ra) >> (32 * c)) & a.mask[c];
                            if (v != 0 || !a.zero_ok[c]) {                         // (v = 0 and zero_ok: found, K ^= 0, P ^= 0)
                                const u64 hit = hash_find<1>(a.tab[c], 0ull, v);
                                if (hit == ~0ull)
                                    unmatched[c] += 1;                             // css_code.py:655-657: no match, nothing recorded
                                else
                                    Ra ^= (v | (u64)(a.flips[c][a.tab[c].val[hit]] & 1u) << 31) << (32 * c);
                            }
                        }
                    }
#pragma unroll
                    for (int q = 0; q < NF; ++q)
                        if (q == fa) R[q] = Ra;
                    if (kind == GF2_STREAM_MEASURE) {
                        const unsigned int bad = (unsigned int)(((word ^ Ra) >> 31) & 1ull);
                        const int m = (info.x >> 8) & 3;
                        wrong_trials += bad << (8 * m);
                        if (info.x & 8) first_wrong |= bad << m;
                    }
                }
                Ta ^= bt;                                                          // (an exhausted lane's frames are never read again)
#pragma unroll
                for (int q = 0; q < NF; ++q)
                    if (q == fa) T[q] = Ta;
            }
        }
        if constexpr (MODE == MG_STORE) row[a.nsteps + a.flag_words] = attempts;
        if constexpr (MODE == MG_TALLY) {
            all_attempts += attempts;
            if (alive) {
                accepted += 1;
                if (unmatched[0]) atomicAdd(&bins[2], unmatched[0]);
                if (unmatched[1]) atomicAdd(&bins[3], unmatched[1]);
                if (wrong_trials) {                                                // (a first trial that is wrong is a wrong trial)
                    unsigned int any = 0;
                    for (int m = 0; m < a.measurements; ++m) {
                        const unsigned int w = (wrong_trials >> (8 * m)) & 255u;
                        if (w == 0) continue;
                        const unsigned int wrong = 2 * w > (unsigned int)a.trials;
                        any |= wrong;
                        if (wrong) atomicAdd(&bins[4 + 4 * m], 1u);
                        atomicAdd(&bins[5 + 4 * m], w);
                        if ((first_wrong >> m) & 1u) atomicAdd(&bins[6 + 4 * m], 1u);
                        if (w != (unsigned int)a.trials) atomicAdd(&bins[7 + 4 * m], 1u);
                    }
                    if (any) atomicAdd(&bins[1], 1u);
                }
            } else {
                atomicAdd(&bins[MG_EXHAUSTED], 1u);
            }
        }
    }
    if constexpr (MODE == MG_TALLY) {
        if (accepted) atomicAdd(&bins[0], accepted);
        if (all_attempts) atomicAdd(attempts_bin, all_attempts);
        __syncthreads();
        if (threadIdx.x < MG_BINS && bins[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (u64)bins[threadIdx.x]);
        if (threadIdx.x == MG_BINS && *attempts_bin) atomicAdd(&a.counts[MG_BINS], *attempts_bin);
    }
}

// A lane adds at most nsteps to a 32-bit field per sample (unmatched keys, wrong trials), a workgroup's 32-bit LDS bins hold the sum
// over its 256 lanes: with at most `per_lane` samples per lane, 256 * per_lane * nsteps must stay below 2^32 (ms_per_lane_cap's
// rule in gf2_mstream.hip).  The attempts are 64-bit throughout and need no such bound.
static int64_t mg_per_lane_cap(int64_t nsteps) { return (int64_t)(0xFFFFFFFFll / (256 * (nsteps > 1 ? nsteps : 1))); }
static_assert(0xFFFFFFFFll / (256ll * (GF2_CIRCUIT_MAX_LOCATIONS + 1)) >= 1, "one sample per lane never wraps a 32-bit bin");

namespace {
struct MRetryGateBuffer {                                                                   // a device buffer of the call's, freed with it
    gf2_ctx* ctx;
    void* dev = nullptr;
    explicit MRetryGateBuffer(gf2_ctx* c) : ctx(c) {}
    ~MRetryGateBuffer() { (void)gf2_dev_free(ctx, dev); }
};
}  // namespace

template <int MODE, int NF>
static int mretry_gate_launch_frames(gf2_ctx* ctx, const gf2_mretry_gate* mr, const MRetryGateArgs& a) {
    const size_t tables = (size_t)mr->table_words * 8 + (size_t)mr->sites * 4;
    const size_t base = (size_t)mr->cdf_words * 8 + 8 + (size_t)CIRC_THREADS * CIRC_TAKEN_STRIDE * 4 + 32 * 4;
    const bool staged = base + tables <= MG_LDS_MAX;
    const size_t lds = base + (staged ? tables : 0);
    // samples per lane: a long program is many segments per sample, so fewer samples per lane keep the grid wide
    int64_t per_lane = 64 / gf2_cdiv(mr->plan.seq.locations, GF2_SEG_BITS);
    if (per_lane > 16) per_lane = 16;
    if (per_lane < 1) per_lane = 1;
    const int64_t cap = mg_per_lane_cap(mr->plan.seq.nsteps);
    if (per_lane > cap) per_lane = cap;
    int64_t blocks = gf2_cdiv(a.count, CIRC_THREADS * per_lane);
    if (blocks > MG_MAX_BLOCKS) blocks = MG_MAX_BLOCKS;                             // (the caller keeps count <= MG_MAX_BLOCKS * 256 * cap)
    if (blocks < 1) blocks = 1;
    if (lds > 64 * 1024) {
        if (staged)
            GF2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mretry_gate_kernel<MODE, true, NF>), hipFuncAttributeMaxDynamicSharedMemorySize, MG_LDS_MAX));
        else
            GF2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mretry_gate_kernel<MODE, false, NF>), hipFuncAttributeMaxDynamicSharedMemorySize, MG_LDS_MAX));
    }
    GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
    if (staged)
        hipLaunchKernelGGL((mretry_gate_kernel<MODE, true, NF>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    else
        hipLaunchKernelGGL((mretry_gate_kernel<MODE, false, NF>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    GF2_TRY(gf2_prof_end(ctx));
    GF2_HIP(hipGetLastError());
    return GF2_OK;
}
// the full tables of GF2_RETRY_MAX_SIZES sizes of both classes, the taken maps, the attempts' bin and the bins fit the budget without
// any block table
static_assert((size_t)2 * GF2_RETRY_MAX_SIZES * GF2_SEG_CDF * 8 + 8 + (size_t)CIRC_THREADS * CIRC_TAKEN_STRIDE * 4 + 32 * 4 <= MG_LDS_MAX, "LDS budget");

template <int MODE>
static int mretry_gate_launch(gf2_ctx* ctx, const gf2_mretry_gate* mr, const MRetryGateArgs& a) {
    const int64_t nframes = mr->plan.nframes;
    if (nframes == 1) return mretry_gate_launch_frames<MODE, 1>(ctx, mr, a);
    if (nframes == 2) return mretry_gate_launch_frames<MODE, 2>(ctx, mr, a);
    return mretry_gate_launch_frames<MODE, 4>(ctx, mr, a);
}

// What a call's kernel arguments take from the handle and the rates, and the call's inverse-CDF tables (made here, uploaded into
// `cdf`, a buffer of the call's).
static int mretry_gate_args(const char* who, gf2_ctx* ctx, const gf2_mretry_gate* mr, uint64_t seed, double p1, double p2, int64_t max_attempts,
                            MRetryGateBuffer* cdf, MRetryGateArgs* a) {
    const uint64_t T[2] = {gf2_quantise(p1), gf2_quantise(p2)};
    std::vector<u64> host;
    try {
        host.resize((size_t)(mr->cdf_words > 0 ? mr->cdf_words : 1));
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    for (int c = 0; c < 2; ++c)
        for (size_t k = 0; k < mr->gate.sizes[c].size(); ++k)
            binomial_cdf_table(T[c], mr->gate.sizes[c][k], host.data() + mr->cdf_off[c][k], mr->gate.sizes[c][k] + 1);
    GF2_TRY(gf2_dev_alloc(ctx, host.size() * 8, &cdf->dev));
    GF2_TRY(gf2_h2d(ctx, cdf->dev, host.data(), host.size() * 8));
    a->cdf = (const u64*)cdf->dev;
    a->cdf_words = mr->cdf_words;
    a->full_off[0] = mr->full_off[0];
    a->full_off[1] = mr->full_off[1];
    a->eff = mr->eff_dev;
    a->site = mr->site_dev;
    a->eff_words = (int)mr->table_words;
    a->sites = (int)mr->sites;
    a->seed = seed;
    a->info = mr->info_dev;
    a->span = mr->span_dev;
    a->region = mr->region_dev;
    a->nblocks = (int)mr->nblocks;
    a->nsteps = (int)mr->plan.seq.nsteps;
    a->flag_words = (int)mr->plan.seq.flag_words;
    a->max_attempts = (int)max_attempts;
    a->trials = (int)mr->plan.seq.trials;
    a->measurements = (int)mr->plan.measurements;
    return GF2_OK;
}

static int mretry_gate_check_attempts(const char* who, int64_t max_attempts) {
    if (max_attempts < 1 || max_attempts > GF2_RETRY_MAX_ATTEMPTS)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= max_attempts <= %d, got %lld", who, GF2_RETRY_MAX_ATTEMPTS, (long long)max_attempts);
    return GF2_OK;
}

extern "C" {

int gf2_mretry_gate_destroy(gf2_ctx* ctx, gf2_mretry_gate* mretry) {
    if (!ctx) GF2_FAIL(GF2_E_ARG, "gf2_mretry_gate_destroy: null context");
    if (!mretry) return GF2_OK;
    GF2_TRY(gf2_ctx_activate(ctx));
    (void)gf2_dev_free(ctx, mretry->eff_dev);
    (void)gf2_dev_free(ctx, mretry->site_dev);
    (void)gf2_dev_free(ctx, mretry->info_dev);
    (void)gf2_dev_free(ctx, mretry->span_dev);
    (void)gf2_dev_free(ctx, mretry->region_dev);
    delete mretry;
    return GF2_OK;
}

int gf2_mretry_gate_create(gf2_ctx* ctx, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                           const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                           int64_t nframes, const int64_t* type_regions, const int64_t* type_nregions, const int32_t* site_loc,
                           const int64_t* site_regions, gf2_mretry_gate** mretry_out) {
    const char* who = "gf2_mretry_gate_create";
    if (!ctx || !mretry_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    *mretry_out = nullptr;
    gf2_mretry_gate* mr = new (std::nothrow) gf2_mretry_gate();
    if (!mr) GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    mr->eff_dev = nullptr, mr->site_dev = nullptr, mr->info_dev = nullptr, mr->span_dev = nullptr, mr->region_dev = nullptr;
    int rc = gf2_mretry_gate_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, block_a, block_b, nblocks, nframes,
                                  type_regions, type_nregions, site_loc, site_regions, 1, &mr->plan, &mr->retry, &mr->gate);
    if (rc != GF2_OK) {
        delete mr;
        return rc;
    }
    const StreamPlan& plan = mr->plan.seq;
    const RetryPlan& retry = mr->retry;
    const RetryGatePlan& gate = mr->gate;
    mr->nblocks = nblocks;
    mr->sites = gate.sites;
    int64_t rows = 0;
    for (int64_t t = 0; t < ntypes; ++t) rows += type_locations[t];
    mr->table_words = rows * 6;
    std::vector<int4> info, region;
    std::vector<int2> span;
    std::vector<int> site;
    try {
        info.resize((size_t)nblocks);
        span.resize((size_t)nblocks);
        region.resize(2 * retry.first.size());
        site.resize((size_t)gate.sites);
        for (int c = 0; c < 2; ++c) mr->cdf_off[c].assign(gate.sizes[c].size(), 0);
    } catch (const std::bad_alloc&) {
        delete mr;
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    int words = 0;
    for (int c = 0; c < 2; ++c) {
        for (size_t k = 0; k < gate.sizes[c].size(); ++k) {
            mr->cdf_off[c][k] = words;
            words += gate.sizes[c][k] + 1;
        }
        mr->full_off[c] = gate.full_size[c] >= 0 ? mr->cdf_off[c][(size_t)gate.full_size[c]] : 0;
    }
    mr->cdf_words = words;
    for (int64_t t = 0; t < ntypes; ++t)
        for (int64_t q = retry.type_first[(size_t)t]; q < retry.type_first[(size_t)t + 1]; ++q) {
            const int n1 = gate.n[0][(size_t)q], n2 = gate.n[1][(size_t)q];
            region[2 * (size_t)q] = make_int4((int)gate.site_first[(size_t)q], n1, n2, retry.retried[(size_t)q]);
            region[2 * (size_t)q + 1] = make_int4(n1 > 0 ? mr->cdf_off[0][(size_t)gate.last_size[0][(size_t)q]] : 0,
                                                  n2 > 0 ? mr->cdf_off[1][(size_t)gate.last_size[1][(size_t)q]] : 0, 0, 0);
            for (int64_t s = gate.site_first[(size_t)q]; s < gate.site_first[(size_t)q] + n1 + n2; ++s)
                site[(size_t)s] = (int)(plan.type_offset[(size_t)t] + site_loc[s]);          // the row in the tables of all types
        }
    for (int64_t b = 0; b < nblocks; ++b) {
        const int kind = block_kind[b];
        const int fb = kind == GF2_MSTREAM_CNOT ? block_b[b] : block_a[b];
        const int m = mr->plan.measure[(size_t)b] < 0 ? 0 : mr->plan.measure[(size_t)b];
        info[(size_t)b] = make_int4(kind | (mr->plan.first_trial[(size_t)b] ? 8 : 0) | block_a[b] << 4 | fb << 6 | m << 8, plan.step[(size_t)b],
                                    plan.flag[(size_t)b], 0);
        span[(size_t)b] = make_int2((int)retry.type_first[(size_t)block_type[b]], (int)retry.type_first[(size_t)block_type[b] + 1]);
    }
    rc = gf2_ctx_activate(ctx);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, (size_t)mr->table_words * 8, (void**)&mr->eff_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, (site.size() + 1) * 4, (void**)&mr->site_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, info.size() * 16, (void**)&mr->info_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, span.size() * 8, (void**)&mr->span_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, region.size() * 16, (void**)&mr->region_dev);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, mr->eff_dev, type_eff, (size_t)mr->table_words * 8);
    if (rc == GF2_OK && !site.empty()) rc = gf2_h2d(ctx, mr->site_dev, site.data(), site.size() * 4);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, mr->info_dev, info.data(), info.size() * 16);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, mr->span_dev, span.data(), span.size() * 8);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, mr->region_dev, region.data(), region.size() * 16);
    if (rc != GF2_OK) {
        (void)gf2_mretry_gate_destroy(ctx, mr);
        return rc;
    }
    *mretry_out = mr;
    return GF2_OK;
}

int gf2_mretry_gate_outcomes_dev(gf2_ctx* ctx, const gf2_mretry_gate* mretry, uint64_t seed, int64_t first_sample, int64_t count, double p1,
                                 double p2, int64_t max_attempts, uint64_t* out_dev, int64_t ldo) {
    const char* who = "gf2_mretry_gate_outcomes_dev";
    if (!ctx || !mretry) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GF2_TRY(mretry_gate_check_attempts(who, max_attempts));
    GF2_TRY(gf2_gate_check_mc(who, p1, p2, first_sample, count));
    const int64_t ldr = mretry->plan.seq.nsteps + mretry->plan.seq.flag_words + 1;
    if (ldo < ldr) GF2_FAIL(GF2_E_ARG, "%s: ldo must be at least the sequence's nsteps + F + 1 = %lld words", who, (long long)ldr);
    if (count == 0) return GF2_OK;
    if (!out_dev) GF2_FAIL(GF2_E_ARG, "%s: null buffer", who);
    GF2_TRY(gf2_ctx_activate(ctx));
    MRetryGateArgs a = {};
    MRetryGateBuffer cdf(ctx);
    GF2_TRY(mretry_gate_args(who, ctx, mretry, seed, p1, p2, max_attempts, &cdf, &a));
    a.ldo = ldo;
    const int64_t most = (int64_t)MG_MAX_BLOCKS * CIRC_THREADS * 16;
    for (int64_t done = 0; done < count; done += most) {
        a.first_sample = first_sample + done;
        a.count = count - done < most ? count - done : most;
        a.out = (u64*)out_dev + done * ldo;
        GF2_TRY((mretry_gate_launch<MG_STORE>(ctx, mretry, a)));
    }
    return gf2_ctx_sync(ctx);                                                      // (the call's tables are freed on return)
}

int gf2_mc_mretry_gate_decode(gf2_ctx* ctx, const gf2_mretry_gate* mretry, int64_t records, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                         int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed,
                         int64_t first_sample, int64_t count, double p1, double p2, int64_t max_attempts, uint64_t* counts_out) {
    const char* who = "gf2_mc_mretry_gate_decode";
    if (!ctx || !mretry || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GF2_TRY(gf2_mstream_check_records(who, records));
    GF2_TRY(gf2_mstream_check_bits(who, mretry->plan, r1, r2));
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    GF2_TRY(mretry_gate_check_attempts(who, max_attempts));
    GF2_TRY(gf2_gate_check_mc(who, p1, p2, first_sample, count));
    GF2_TRY(gf2_ctx_activate(ctx));
    for (int k = 0; k < MG_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    MRetryGateArgs a = {};
    MRetryGateBuffer cdf(ctx);
    GF2_TRY(mretry_gate_args(who, ctx, mretry, seed, p1, p2, max_attempts, &cdf, &a));
    a.propagated = records == GF2_MSTREAM_PROPAGATED;
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
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, MG_FIELDS, &a));
    a.counts = tables.counts_dev;
    const int64_t most = (int64_t)MG_MAX_BLOCKS * CIRC_THREADS * mg_per_lane_cap(mretry->plan.seq.nsteps);
    for (int64_t done = 0; done < count; done += most) {
        a.first_sample = first_sample + done;
        a.count = count - done < most ? count - done : most;
        GF2_TRY((mretry_gate_launch<MG_TALLY>(ctx, mretry, a)));
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, MG_FIELDS * 8);              // (waits for the launches: the call's tables are freed on return)
}

}  // extern "C"
