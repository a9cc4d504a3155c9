// Repeat-until-success Monte-Carlo with waiting faults on the data block (DESIGN.md section 5d "Repeat-until-success with waiting
// faults", include/gf2hip.h).  gf2_retry.hip redraws a preparation until its verifications pass and lets the data block wait through
// the retries for nothing.  Here every attempt made of a retried region, the failed ones included, also draws the region's wait rows
// -- the qubits of the data block that no gate of the region touches -- with a memory error rate of their own.
//
// retry_kernel's structure stands: lane = sample, uniform block and region loops, one divergent attempt loop.  Inside that loop,
// after the region's own draw, comes the wait draw: one error_count under the wait key of (region, attempt), usually K = 0.  Its
// picks go into a second pair of accumulators per lane (wait local, wait tail) that no attempt clears and that are folded into the
// block's words when the region ends.  The taken map is free again by then and is used for both draws.  The wait key and the region's
// key are separate streams, so the attempts of every preparation are those gf2_retry.hip makes.
//
// Tally: retry_kernel's, plus the wait faults drawn over all attempts, 64-bit per lane, per workgroup and per call as the attempts are.
//
// LDS per workgroup: the packed inverse-CDF tables of the regions' segment sizes and of the wait sizes (made per call from p and q),
// the wait tables (4 words per row) when they fit after those, the block types' tables when all of that still fits RW_LDS_MAX --
// otherwise either is read through L2 --, two 64-bit bins, the taken maps and the 32-bit bins.
#include <limits.h>

#include <new>
#include <vector>

#include "gf2_internal.h"
#include "gf2_circuit_dev.h"
#include "gf2_retry_wait_plan.h"

#define RW_FIELDS GF2_RETRY_WAIT_FIELDS
#define RW_BINS 13                              // the 32-bit bins: every field but the attempts and the wait faults
#define RW_LDS_MAX (160 * 1024)                 // gf2_retry.hip's budget
#define RW_MAX_BLOCKS 4096
#define RW_FIRST_MEASURE 4                      // bit of RetryWaitArgs::info[b].x beside the kind

static_assert(RW_FIELDS == GF2_RETRY_FIELDS + 1 && GF2_RETRY_FIELDS == RW_BINS + 1, "the retried fields, then the wait faults");

enum { RW_STORE = 0, RW_TALLY = 1 };

struct gf2_retry_wait {
    StreamPlan plan;
    RetryPlan retry;
    RetryWaitPlan wait;
    int64_t nblocks, table_words, wait_words;  // blocks, the FINAL step included; words of all types' tables; of all wait rows
    int cdf_words, full_off, wcdf_words;       // words of the packed inverse-CDF tables; where the table of nb = 512 starts; of the wait sizes' tables
    std::vector<int> cdf_off, wcdf_off;        // where the table of every distinct size starts
    u64* eff_dev;
    u64* wait_dev;                             // the wait rows (at least one word)
    int4* info_dev;                            // nblocks: (kind | RW_FIRST_MEASURE, step or -1, first flag row, 0)
    int2* span_dev;                            // nblocks: the block's regions [first, end) among region_dev
    int4* region_dev;                          // per region of every type: (first table row, locations, retried, its last segment's table)
    int4* wregion_dev;                         // per region of every type: (first wait row, wait rows, their table, 0)
};

struct RetryWaitArgs {
    const u64* eff;
    const u64* wait_eff;
    int eff_words, wait_words, wait_lds;       // wait_lds: the wait rows are staged
    u64 seed;
    int64_t first_sample, count;
    u64 t_1, t_2, w_1, w_2;                    // the kinds' thresholds of p and of q
    const u64* cdf;                            // the tables of p, then those of q
    int cdf_words, full_off, wcdf_words;
    const int4* info;
    const int2* span;
    const int4* region;
    const int4* wregion;
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
__global__ __launch_bounds__(CIRC_THREADS) void retry_wait_kernel(RetryWaitArgs a) {
    extern __shared__ u64 rw_lds[];
    u64* cdf_lds = rw_lds;                                                         // the packed tables of p
    u64* wcdf_lds = cdf_lds + a.cdf_words;                                         // ... and of q
    u64* weff_lds = wcdf_lds + a.wcdf_words;
    u64* eff_lds = weff_lds + (a.wait_lds ? a.wait_words : 0);
    u64* wide_bins = eff_lds + (STAGED ? a.eff_words : 0);                         // [0]: attempts, [1]: wait faults
    unsigned int* taken = (unsigned int*)(wide_bins + 2);
    unsigned int* bins = taken + CIRC_THREADS * CIRC_TAKEN_STRIDE;                 // RW_BINS
    for (int i = threadIdx.x; i < a.cdf_words + a.wcdf_words; i += blockDim.x) cdf_lds[i] = a.cdf[i];
    if (a.wait_lds)
        for (int i = threadIdx.x; i < a.wait_words; i += blockDim.x) weff_lds[i] = a.wait_eff[i];
    if (STAGED)
        for (int i = threadIdx.x; i < a.eff_words; i += blockDim.x) eff_lds[i] = a.eff[i];
    if (MODE == RW_TALLY && threadIdx.x < RW_BINS) bins[threadIdx.x] = 0;
    if (MODE == RW_TALLY && threadIdx.x < 2) wide_bins[threadIdx.x] = 0;
    __syncthreads();
    const u64* eff = STAGED ? eff_lds : a.eff;
    unsigned int* mine = taken + threadIdx.x * CIRC_TAKEN_STRIDE;
    unsigned int local[RW_BINS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    u64 all_attempts = 0, all_waited = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += stride) {
        const u64 ks = sample_key(a.seed, (u64)(a.first_sample + i));
        u64 T = 0, K[2] = {0, 0};                                                  // the data frame; syndrome of the errors recorded so far, per side
        unsigned int P[2] = {0, 0}, unmatched[2] = {0, 0};                         // ... and their operator parity
        unsigned int wrong_trials = 0, first_wrong = 0, final_bits = 0;           // final_bits: flip_x, flip_z, miss_x, miss_z
        u64 attempts = 0, waited = 0;
        u64* row = MODE == RW_STORE ? a.out + i * a.ldo : nullptr;
        if constexpr (MODE == RW_STORE)
            for (int q = 0; q < a.flag_words; ++q) row[a.nsteps + q] = 0;
        bool alive = true;
        u64 g = 0;                                                                 // the region's number in the whole sequence (uniform)
        for (int b = 0; b < a.nblocks; ++b) {
            const int4 info = a.info[b];
            const int2 span = a.span[b];
            u64 bl = 0, bt = 0;                                                    // the block's local and tail words
            for (int r = span.x; r < span.y; ++r, ++g) {
                const int4 reg = a.region[r];
                const int4 wreg = a.wregion[r];
                if (alive) {
                    const u64 kr = segment_draw(ks, GF2_RETRY_SLOT_BASE + g);
                    const u64 kw = wreg.y > 0 ? segment_draw(ks, GF2_RETRY_WAIT_SLOT_BASE + g) : 0ull;   // (uniform: only a region that has wait rows pays)
                    const int limit = reg.z ? a.max_attempts : 1;
                    const int nseg = (reg.y + GF2_SEG_BITS - 1) / GF2_SEG_BITS;
                    u64 l, t, f, wl = 0, wt = 0;                                   // wl, wt: what the data picked up while it waited, never cleared
                    int att = 0;
                    do {                                                           // the one divergent loop
                        const u64 ka = mix64(kr + GF2_GOLDEN * (u64)(att + 1));
                        l = t = f = 0;
                        for (int s = 0; s < nseg; ++s) {
                            const bool last = s == nseg - 1;
                            const int nb = last ? reg.y - s * GF2_SEG_BITS : GF2_SEG_BITS;
                            const u64 d = segment_draw(ka, (u64)s);
                            const int Kn = error_count(d, nb, cdf_lds + (last ? reg.w : a.full_off));
                            if (Kn > 1)
                                for (int w = 0; w < (nb + 31) >> 5; ++w) mine[w] = 0;
                            for (int k = 0; k < Kn; ++k) {
                                unsigned int pick, kind;
                                error_draw(d, k, Kn, nb, a.t_1, a.t_2, &pick, &kind);
                                unsigned int pos = pick;
                                if (Kn > 1) {                                      // Floyd's rule: a candidate already taken -> j
                                    if ((mine[pick >> 5] >> (pick & 31u)) & 1u) pos = (unsigned int)(nb - Kn + k);
                                    mine[pos >> 5] |= 1u << (pos & 31u);
                                }
                                const u64* e = eff + (size_t)(reg.x + s * GF2_SEG_BITS + (int)pos) * 6;   // pos < nb: a row of the region
                                if (kind & 1u) l ^= e[0], t ^= e[1], f ^= e[2];
                                if (kind & 2u) l ^= e[3], t ^= e[4], f ^= e[5];
                            }
                        }
                        if (wreg.y > 0) {                                          // the data waits through this attempt, passed or not
                            const u64 d = segment_draw(mix64(kw + GF2_GOLDEN * (u64)(att + 1)), 0ull);
                            const int Kn = error_count(d, wreg.y, wcdf_lds + wreg.z);
                            if (Kn > 1)
                                for (int w = 0; w < (wreg.y + 31) >> 5; ++w) mine[w] = 0;
                            for (int k = 0; k < Kn; ++k) {
                                unsigned int pick, kind;
                                error_draw(d, k, Kn, wreg.y, a.w_1, a.w_2, &pick, &kind);
                                unsigned int pos = pick;
                                if (Kn > 1) {
                                    if ((mine[pick >> 5] >> (pick & 31u)) & 1u) pos = (unsigned int)(wreg.y - Kn + k);
                                    mine[pos >> 5] |= 1u << (pos & 31u);
                                }
                                const size_t at = (size_t)(wreg.x + (int)pos) * 4;  // pos < wreg.y: a wait row of the region
                                u64 xl, xt, zl, zt;
                                if (a.wait_lds)
                                    xl = weff_lds[at], xt = weff_lds[at + 1], zl = weff_lds[at + 2], zt = weff_lds[at + 3];
                                else
                                    xl = a.wait_eff[at], xt = a.wait_eff[at + 1], zl = a.wait_eff[at + 2], zt = a.wait_eff[at + 3];
                                if (kind & 1u) wl ^= xl, wt ^= xt;
                                if (kind & 2u) wl ^= zl, wt ^= zt;
                            }
                            waited += (u64)Kn;
                        }
                        att += 1;
                    } while (f != 0 && att < limit);
                    if (reg.z) attempts += (u64)att;
                    if (f != 0) {                                                  // no attempt passed: the sample is exhausted
                        alive = false;
                        if constexpr (MODE == RW_STORE) {
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
            if constexpr (MODE == RW_STORE) {
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
                                    unmatched[c] += 1;                             // css_code.py:655-657: no match, nothing recorded
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
                        if (info.x & RW_FIRST_MEASURE) first_wrong = bad;
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
        if constexpr (MODE == RW_STORE) {
            row[a.nsteps + a.flag_words] = attempts;
            row[a.nsteps + a.flag_words + 1] = waited;
        }
        if constexpr (MODE == RW_TALLY) {
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
    if constexpr (MODE == RW_TALLY) {
#pragma unroll
        for (int k = 0; k < RW_BINS; ++k)
            if (local[k]) atomicAdd(&bins[k], local[k]);
        if (all_attempts) atomicAdd(&wide_bins[0], all_attempts);
        if (all_waited) atomicAdd(&wide_bins[1], all_waited);
        __syncthreads();
        if (threadIdx.x < RW_BINS && bins[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (u64)bins[threadIdx.x]);
        if (threadIdx.x >= RW_BINS && threadIdx.x < RW_FIELDS && wide_bins[threadIdx.x - RW_BINS])
            atomicAdd(&a.counts[threadIdx.x], wide_bins[threadIdx.x - RW_BINS]);
    }
}

// gf2_retry.hip's rule: with at most `per_lane` samples per lane, 256 * per_lane * nsteps must stay below 2^32 for the 32-bit bins.
// The attempts and the wait faults are 64-bit throughout and need no such bound.
static int64_t rw_per_lane_cap(int64_t nsteps) { return (int64_t)(0xFFFFFFFFll / (256 * (nsteps > 1 ? nsteps : 1))); }

namespace {
struct RetryWaitBuffer {                                                                // a device buffer of the call's, freed with it
    gf2_ctx* ctx;
    void* dev = nullptr;
    explicit RetryWaitBuffer(gf2_ctx* c) : ctx(c) {}
    ~RetryWaitBuffer() { (void)gf2_dev_free(ctx, dev); }
};
}  // namespace

// What of the budget the tables of both rates, the two wide bins, the taken maps and the 32-bit bins take
static size_t rw_lds_base(const gf2_retry_wait* rt) {
    return (size_t)(rt->cdf_words + rt->wcdf_words) * 8 + 16 + (size_t)CIRC_THREADS * CIRC_TAKEN_STRIDE * 4 + 16 * 4;
}
static bool rw_wait_staged(const gf2_retry_wait* rt) { return rw_lds_base(rt) + (size_t)rt->wait_words * 8 <= RW_LDS_MAX; }
// the tables of GF2_RETRY_MAX_SIZES sizes of either rate, the taken maps and the bins fit the budget without any other table
static_assert((size_t)2 * GF2_RETRY_MAX_SIZES * GF2_SEG_CDF * 8 + 16 + (size_t)CIRC_THREADS * CIRC_TAKEN_STRIDE * 4 + 16 * 4 <= RW_LDS_MAX, "LDS budget");

template <int MODE>
static int retry_wait_launch(gf2_ctx* ctx, const gf2_retry_wait* rt, const RetryWaitArgs& a) {
    const size_t eff_bytes = (size_t)rt->table_words * 8;
    const size_t base = rw_lds_base(rt) + (a.wait_lds ? (size_t)rt->wait_words * 8 : 0);
    const bool staged = base + eff_bytes <= RW_LDS_MAX;
    const size_t lds = base + (staged ? eff_bytes : 0);
    // samples per lane: a long gadget is many segments per sample, so fewer samples per lane keep the grid wide
    int64_t per_lane = 64 / gf2_cdiv(rt->plan.locations, GF2_SEG_BITS);
    if (per_lane > 16) per_lane = 16;
    if (per_lane < 1) per_lane = 1;
    const int64_t cap = rw_per_lane_cap(rt->plan.nsteps);
    if (per_lane > cap) per_lane = cap;
    int64_t blocks = gf2_cdiv(a.count, CIRC_THREADS * per_lane);
    if (blocks > RW_MAX_BLOCKS) blocks = RW_MAX_BLOCKS;                             // (the caller keeps count <= RW_MAX_BLOCKS * 256 * cap)
    if (blocks < 1) blocks = 1;
    if (lds > 64 * 1024) {
        if (staged)
            GF2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(retry_wait_kernel<MODE, true>), hipFuncAttributeMaxDynamicSharedMemorySize, RW_LDS_MAX));
        else
            GF2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(retry_wait_kernel<MODE, false>), hipFuncAttributeMaxDynamicSharedMemorySize, RW_LDS_MAX));
    }
    GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
    if (staged)
        hipLaunchKernelGGL((retry_wait_kernel<MODE, true>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    else
        hipLaunchKernelGGL((retry_wait_kernel<MODE, false>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    GF2_TRY(gf2_prof_end(ctx));
    GF2_HIP(hipGetLastError());
    return GF2_OK;
}

// What a call's kernel arguments take from the handle and the rates, and the call's inverse-CDF tables of p and of q (made here,
// uploaded into `cdf`, a buffer of the call's).
static int retry_wait_args(const char* who, gf2_ctx* ctx, const gf2_retry_wait* rt, uint64_t seed, double p_x, double p_y, double p_z, double q_x,
                           double q_y, double q_z, int64_t max_attempts, RetryWaitBuffer* cdf, RetryWaitArgs* a) {
    const double p_t = p_x + p_y + p_z, q_t = q_x + q_y + q_z;
    const uint64_t t_any = gf2_quantise(p_t), w_any = gf2_quantise(q_t);
    a->t_1 = p_t > 0.0 ? gf2_quantise(p_x / p_t) : 0;
    a->t_2 = p_t > 0.0 ? gf2_quantise((p_x + p_y) / p_t) : 0;
    a->w_1 = q_t > 0.0 ? gf2_quantise(q_x / q_t) : 0;
    a->w_2 = q_t > 0.0 ? gf2_quantise((q_x + q_y) / q_t) : 0;
    std::vector<u64> host;
    try {
        host.resize((size_t)(rt->cdf_words + rt->wcdf_words) + 1);               // (never empty)
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    for (size_t k = 0; k < rt->retry.sizes.size(); ++k)
        binomial_cdf_table(t_any, rt->retry.sizes[k], host.data() + rt->cdf_off[k], rt->retry.sizes[k] + 1);
    for (size_t k = 0; k < rt->wait.sizes.size(); ++k)
        binomial_cdf_table(w_any, rt->wait.sizes[k], host.data() + rt->cdf_words + rt->wcdf_off[k], rt->wait.sizes[k] + 1);
    GF2_TRY(gf2_dev_alloc(ctx, host.size() * 8, &cdf->dev));
    GF2_TRY(gf2_h2d(ctx, cdf->dev, host.data(), host.size() * 8));
    a->cdf = (const u64*)cdf->dev;
    a->cdf_words = rt->cdf_words;
    a->wcdf_words = rt->wcdf_words;
    a->full_off = rt->full_off;
    a->eff = rt->eff_dev;
    a->eff_words = (int)rt->table_words;
    a->wait_eff = rt->wait_dev;
    a->wait_words = (int)rt->wait_words;
    a->wait_lds = rw_wait_staged(rt) ? 1 : 0;
    a->seed = seed;
    a->info = rt->info_dev;
    a->span = rt->span_dev;
    a->region = rt->region_dev;
    a->wregion = rt->wregion_dev;
    a->nblocks = (int)rt->nblocks;
    a->nsteps = (int)rt->plan.nsteps;
    a->flag_words = (int)rt->plan.flag_words;
    a->max_attempts = (int)max_attempts;
    a->trials = (int)rt->plan.trials;
    return GF2_OK;
}

static int retry_wait_check_call(const char* who, int64_t max_attempts, double p_x, double p_y, double p_z, double q_x, double q_y, double q_z,
                                 int64_t first_sample, int64_t count) {
    if (max_attempts < 1 || max_attempts > GF2_RETRY_MAX_ATTEMPTS)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= max_attempts <= %d, got %lld", who, GF2_RETRY_MAX_ATTEMPTS, (long long)max_attempts);
    GF2_TRY(gf2_retry_check_range(who, p_x, p_y, p_z, first_sample, count));
    return gf2_retry_wait_check_rates(who, q_x, q_y, q_z);
}

extern "C" {

int gf2_retry_wait_destroy(gf2_ctx* ctx, gf2_retry_wait* retry) {
    if (!ctx) GF2_FAIL(GF2_E_ARG, "gf2_retry_wait_destroy: null context");
    if (!retry) return GF2_OK;
    GF2_TRY(gf2_ctx_activate(ctx));
    (void)gf2_dev_free(ctx, retry->eff_dev);
    (void)gf2_dev_free(ctx, retry->wait_dev);
    (void)gf2_dev_free(ctx, retry->info_dev);
    (void)gf2_dev_free(ctx, retry->span_dev);
    (void)gf2_dev_free(ctx, retry->region_dev);
    (void)gf2_dev_free(ctx, retry->wregion_dev);
    delete retry;
    return GF2_OK;
}

int gf2_retry_wait_create(gf2_ctx* ctx, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                          const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                          const int64_t* type_nregions, const uint64_t* wait_eff, const int64_t* wait_count, gf2_retry_wait** retry_out) {
    const char* who = "gf2_retry_wait_create";
    if (!ctx || !retry_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    *retry_out = nullptr;
    gf2_retry_wait* rt = new (std::nothrow) gf2_retry_wait();
    if (!rt) GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    rt->eff_dev = rt->wait_dev = nullptr, rt->info_dev = nullptr, rt->span_dev = nullptr, rt->region_dev = rt->wregion_dev = nullptr;
    int rc = gf2_retry_wait_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, nblocks, type_regions, type_nregions,
                                 wait_eff, wait_count, 1, &rt->plan, &rt->retry, &rt->wait);
    if (rc != GF2_OK) {
        delete rt;
        return rc;
    }
    const StreamPlan& plan = rt->plan;
    const RetryPlan& retry = rt->retry;
    const RetryWaitPlan& wait = rt->wait;
    rt->nblocks = nblocks;
    int64_t rows = 0;
    for (int64_t t = 0; t < ntypes; ++t) rows += type_locations[t];
    rt->table_words = rows * 6;
    rt->wait_words = wait.rows * 4;
    std::vector<int4> info, region, wregion;
    std::vector<int2> span;
    try {
        info.resize((size_t)nblocks);
        span.resize((size_t)nblocks);
        region.resize(retry.first.size());
        wregion.resize(retry.first.size());
        rt->cdf_off.assign(retry.sizes.size(), 0);
        rt->wcdf_off.assign(wait.sizes.size(), 0);
    } catch (const std::bad_alloc&) {
        delete rt;
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    int words = 0;
    for (size_t k = 0; k < retry.sizes.size(); ++k) {
        rt->cdf_off[k] = words;
        words += retry.sizes[k] + 1;
    }
    rt->cdf_words = words;
    rt->full_off = retry.full_size >= 0 ? rt->cdf_off[(size_t)retry.full_size] : 0;
    words = 0;
    for (size_t k = 0; k < wait.sizes.size(); ++k) {
        rt->wcdf_off[k] = words;
        words += wait.sizes[k] + 1;
    }
    rt->wcdf_words = words;
    for (int64_t t = 0; t < ntypes; ++t)
        for (int64_t q = retry.type_first[(size_t)t]; q < retry.type_first[(size_t)t + 1]; ++q) {
            region[(size_t)q] = make_int4((int)(plan.type_offset[(size_t)t] + retry.first[(size_t)q]), retry.count[(size_t)q], retry.retried[(size_t)q],
                                          rt->cdf_off[(size_t)retry.last_size[(size_t)q]]);
            wregion[(size_t)q] = make_int4((int)wait.first[(size_t)q], wait.count[(size_t)q],
                                           wait.count[(size_t)q] > 0 ? rt->wcdf_off[(size_t)wait.size[(size_t)q]] : 0, 0);
        }
    bool seen_measure = false;
    for (int64_t b = 0; b < nblocks; ++b) {
        const int kind = block_kind[b];
        info[(size_t)b] = make_int4(kind | (kind == GF2_STREAM_MEASURE && !seen_measure ? RW_FIRST_MEASURE : 0), plan.step[(size_t)b], plan.flag[(size_t)b], 0);
        seen_measure |= kind == GF2_STREAM_MEASURE;
        span[(size_t)b] = kind == GF2_STREAM_FINAL ? make_int2(0, 0)
                                                   : make_int2((int)retry.type_first[(size_t)block_type[b]], (int)retry.type_first[(size_t)block_type[b] + 1]);
    }
    const size_t wait_bytes = (size_t)(rt->wait_words > 0 ? rt->wait_words : 1) * 8;
    rc = gf2_ctx_activate(ctx);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, (size_t)rt->table_words * 8, (void**)&rt->eff_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, wait_bytes, (void**)&rt->wait_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, info.size() * 16, (void**)&rt->info_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, span.size() * 8, (void**)&rt->span_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, region.size() * 16, (void**)&rt->region_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, wregion.size() * 16, (void**)&rt->wregion_dev);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->eff_dev, type_eff, (size_t)rt->table_words * 8);
    if (rc == GF2_OK && rt->wait_words > 0) rc = gf2_h2d(ctx, rt->wait_dev, wait_eff, (size_t)rt->wait_words * 8);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->info_dev, info.data(), info.size() * 16);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->span_dev, span.data(), span.size() * 8);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->region_dev, region.data(), region.size() * 16);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, rt->wregion_dev, wregion.data(), wregion.size() * 16);
    if (rc != GF2_OK) {
        (void)gf2_retry_wait_destroy(ctx, rt);
        return rc;
    }
    *retry_out = rt;
    return GF2_OK;
}

int gf2_retry_wait_outcomes_dev(gf2_ctx* ctx, const gf2_retry_wait* retry, uint64_t seed, int64_t first_sample, int64_t count, double p_x,
                                double p_y, double p_z, double q_x, double q_y, double q_z, int64_t max_attempts, uint64_t* out_dev,
                                int64_t ldo) {
    const char* who = "gf2_retry_wait_outcomes_dev";
    if (!ctx || !retry) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GF2_TRY(retry_wait_check_call(who, max_attempts, p_x, p_y, p_z, q_x, q_y, q_z, first_sample, count));
    const int64_t ldr = retry->plan.nsteps + retry->plan.flag_words + 2;
    if (ldo < ldr) GF2_FAIL(GF2_E_ARG, "%s: ldo must be at least the sequence's nsteps + F + 2 = %lld words", who, (long long)ldr);
    if (count == 0) return GF2_OK;
    if (!out_dev) GF2_FAIL(GF2_E_ARG, "%s: null buffer", who);
    GF2_TRY(gf2_ctx_activate(ctx));
    RetryWaitArgs a = {};
    RetryWaitBuffer cdf(ctx);
    GF2_TRY(retry_wait_args(who, ctx, retry, seed, p_x, p_y, p_z, q_x, q_y, q_z, max_attempts, &cdf, &a));
    a.ldo = ldo;
    const int64_t most = (int64_t)RW_MAX_BLOCKS * CIRC_THREADS * 16;
    for (int64_t done = 0; done < count; done += most) {
        a.first_sample = first_sample + done;
        a.count = count - done < most ? count - done : most;
        a.out = (u64*)out_dev + done * ldo;
        GF2_TRY((retry_wait_launch<RW_STORE>(ctx, retry, a)));
    }
    return gf2_ctx_sync(ctx);                                                      // (the call's tables are freed on return)
}

int gf2_mc_retry_wait_decode(gf2_ctx* ctx, const gf2_retry_wait* retry, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                             int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed,
                             int64_t first_sample, int64_t count, double p_x, double p_y, double p_z, double q_x, double q_y, double q_z,
                             int64_t max_attempts, uint64_t* counts_out) {
    const char* who = "gf2_mc_retry_wait_decode";
    if (!ctx || !retry || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GF2_TRY(gf2_stream_check_bits(who, retry->plan, r1, r2));                       // (the plan holds the wait rows' bits too)
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    GF2_TRY(retry_wait_check_call(who, max_attempts, p_x, p_y, p_z, q_x, q_y, q_z, first_sample, count));
    GF2_TRY(gf2_ctx_activate(ctx));
    for (int k = 0; k < RW_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    RetryWaitArgs a = {};
    RetryWaitBuffer cdf(ctx);
    GF2_TRY(retry_wait_args(who, ctx, retry, seed, p_x, p_y, p_z, q_x, q_y, q_z, max_attempts, &cdf, &a));
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
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, RW_FIELDS, &a));
    a.counts = tables.counts_dev;
    const int64_t most = (int64_t)RW_MAX_BLOCKS * CIRC_THREADS * rw_per_lane_cap(retry->plan.nsteps);
    for (int64_t done = 0; done < count; done += most) {
        a.first_sample = first_sample + done;
        a.count = count - done < most ? count - done : most;
        GF2_TRY((retry_wait_launch<RW_TALLY>(ctx, retry, a)));
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, RW_FIELDS * 8);              // (waits for the launches: the call's tables are freed on return)
}

}  // extern "C"
