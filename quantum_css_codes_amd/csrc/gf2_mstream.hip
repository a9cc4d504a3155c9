// Multi-block streamed programs (DESIGN.md section 5d "Multi-block programs", include/gf2hip.h): rewritten programs on up to four
// logical qubits with the transversal CNOT, walked block by block.  gf2_stream.hip's walk with one data frame T per logical qubit:
// a block of the kinds NONE, EC and MEASURE serves frame a by the streamed rule, a CNOT block applies the frame map
//     T_b ^= T_a & 0x00000000FFFFFFFF;   T_a ^= T_b & 0xFFFFFFFF00000000
// to the two carried words and then XORs its faults' two tails.  Time and memory per sample stay linear in the number of blocks.
//
// Lane = sample; the sampler, the accumulator slots of the blocks a segment overlaps and the closing of blocks in order are
// gf2_stream.hip's, draw for draw.  A CNOT block's accumulator holds (tail for a, tail for b, 0) where another block's holds (local,
// tail, flags), so there is no fourth accumulator.
//
// Tally: one record per data frame, packed as the frame is -- R = K_x | P_x << 31 | K_z << 32 | P_z << 63 -- so an EC or MEASURE step
// updates R_a by the streamed rule and GF2_MSTREAM_PROPAGATED is the frame map on (R_a, R_b).  T[NF] and R[NF] never take a run-time
// index: the frames a and b of a block are uniform, and the words are picked and put back through chains of selects over
// compile-time indices (gf2_ec.hip's header says why).  The kernels are instantiated on NF in {1, 2, 4} frames (three frames run as
// four) and use no scratch (DESIGN.md has the build's figures).  Only `accepted` is counted in a register; the other nineteen
// fields are rare events and go to the workgroup's LDS bins directly.
//
// LDS per workgroup: the sampler's two inverse-CDF tables, the taken maps, the twenty counts, and the block types' tables when all
// of that fits 160 KiB; otherwise the tables are read through L2.
#include <limits.h>

#include <new>
#include <vector>

#include "gf2_internal.h"
#include "gf2_circuit_dev.h"
#include "gf2_mstream_plan.h"

#define MS_NACC GF2_STREAM_MAX_OVERLAP
#define MS_FIELDS GF2_MSTREAM_FIELDS
#define MS_LDS_MAX (160 * 1024)
#define MS_MAX_BLOCKS 4096
#define MS_LOW 0x00000000FFFFFFFFull
#define MS_HIGH 0xFFFFFFFF00000000ull

enum { MS_STORE = 0, MS_TALLY = 1 };

struct gf2_mstream {
    MStreamPlan plan;
    int64_t nblocks, table_words;              // blocks; words of all types' tables
    u64* eff_dev;
    int* start_dev;                            // nblocks + 1 first locations (the last: L), then MS_NACC + 1 times INT_MAX
    int* delta_dev;                            // nblocks + MS_NACC: the type's first table row - the block's first location (pads 0)
    int4* info_dev;                            // nblocks: (kind | first trial << 3 | a << 4 | b << 6 | measurement << 8, step or -1, first flag row, 0)
};

struct MStreamArgs {
    const u64* eff;
    int eff_words;
    u64 seed;
    int64_t first_sample, count;
    SegTables th;
    const int* start;
    const int* delta;
    const int4* info;
    int nblocks, locations, nsteps, flag_words;
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
__global__ __launch_bounds__(CIRC_THREADS) void mstream_kernel(MStreamArgs a) {
    extern __shared__ u64 ms_lds[];
    u64* cdf_lds = ms_lds;                                                         // [2][GF2_SEG_CDF]
    u64* eff_lds = ms_lds + 2 * GF2_SEG_CDF;
    unsigned int* taken = (unsigned int*)(eff_lds + (STAGED ? a.eff_words : 0));
    unsigned int* bins = taken + CIRC_THREADS * CIRC_TAKEN_STRIDE;                 // MS_FIELDS
    for (int i = threadIdx.x; i < 2 * GF2_SEG_CDF; i += blockDim.x)
        if (a.th.nseg > 1 || i >= GF2_SEG_CDF) cdf_lds[i] = a.th.cdf[i];            // (one segment: only the last one's table is read)
    if (STAGED)
        for (int i = threadIdx.x; i < a.eff_words; i += blockDim.x) eff_lds[i] = a.eff[i];
    if (MODE == MS_TALLY && threadIdx.x < MS_FIELDS) bins[threadIdx.x] = 0;
    __syncthreads();
    const u64* eff = STAGED ? eff_lds : a.eff;
    unsigned int* mine = taken + threadIdx.x * CIRC_TAKEN_STRIDE;
    unsigned int accepted = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += stride) {
        const u64 ks = sample_key(a.seed, (u64)(a.first_sample + i));
        u64 T[NF], R[NF];                                                          // the data frames; the records, packed as a frame is
#pragma unroll
        for (int q = 0; q < NF; ++q) T[q] = R[q] = 0;
        unsigned int unmatched[2] = {0, 0};
        unsigned int wrong_trials = 0, first_wrong = 0;                            // a byte per measurement; a bit per measurement
        u64 acc_l[MS_NACC], acc_t[MS_NACC], acc_f[MS_NACC];                        // slot j: block lo + j
#pragma unroll
        for (int j = 0; j < MS_NACC; ++j) acc_l[j] = acc_t[j] = acc_f[j] = 0;
        u64* row = MODE == MS_STORE ? a.out + i * a.ldo : nullptr;
        if constexpr (MODE == MS_STORE)
            for (int q = 0; q < a.flag_words; ++q) row[a.nsteps + q] = 0;
        int lo = 0;
        bool alive = true;
        for (int s = 0; s < a.th.nseg && alive; ++s) {
            const bool last = s == a.th.nseg - 1;
            const int nb = last ? a.th.nb_last : GF2_SEG_BITS;
            const int seg_end = s * GF2_SEG_BITS + nb;
            const u64 d = segment_draw(ks, (u64)s);
            const int Kn = error_count(d, nb, cdf_lds + (last ? GF2_SEG_CDF : 0));
            if (Kn > 0) {
                int st[MS_NACC], dl[MS_NACC];                                      // uniform: constant indices only
#pragma unroll
                for (int j = 0; j < MS_NACC; ++j) st[j] = a.start[lo + j], dl[j] = a.delta[lo + j];
                if (Kn > 1)
                    for (int w = 0; w < (nb + 31) >> 5; ++w) mine[w] = 0;
                for (int k = 0; k < Kn; ++k) {
                    unsigned int t, kind;
                    error_draw(d, k, Kn, nb, a.th.t_1, a.th.t_2, &t, &kind);
                    unsigned int pos = t;
                    if (Kn > 1) {                                                  // Floyd's rule: a candidate already taken -> j
                        if ((mine[t >> 5] >> (t & 31u)) & 1u) pos = (unsigned int)(nb - Kn + k);
                        mine[pos >> 5] |= 1u << (pos & 31u);
                    }
                    const int g = s * GF2_SEG_BITS + (int)pos;                     // pos < nb: a location below L
                    int slot = 0, base = dl[0];
#pragma unroll
                    for (int j = 1; j < MS_NACC; ++j)
                        if (g >= st[j]) slot = j, base = dl[j];                    // (the pads are INT_MAX: never taken)
                    const u64* e = eff + (size_t)(base + g) * 6;                   // base + g: a row of the block's type, below the tables' end
                    u64 vl = 0, vt = 0, vf = 0;
                    if (kind & 1u) vl ^= e[0], vt ^= e[1], vf ^= e[2];
                    if (kind & 2u) vl ^= e[3], vt ^= e[4], vf ^= e[5];
#pragma unroll
                    for (int j = 0; j < MS_NACC; ++j)
                        if (slot == j) acc_l[j] ^= vl, acc_t[j] ^= vt, acc_f[j] ^= vf;
                }
            }
            // close the blocks that end in this segment, in order (all of it uniform but the lanes' own words)
            int closed = 0;
#pragma unroll 1
            while (closed < MS_NACC && lo + closed < a.nblocks && a.start[lo + closed + 1] <= seg_end) {
                u64 l = 0, t = 0, f = 0;
#pragma unroll
                for (int j = 0; j < MS_NACC; ++j)
                    if (j == closed) l = acc_l[j], t = acc_t[j], f = acc_f[j];
                const int4 info = a.info[lo + closed];
                const int kind = info.x & 7, fa = (info.x >> 4) & 3, fb = (info.x >> 6) & 3;
                u64 Ta = 0, Tb = 0;
#pragma unroll
                for (int q = 0; q < NF; ++q) {
                    if (q == fa) Ta = T[q];
                    if (q == fb) Tb = T[q];
                }
                if (kind == GF2_MSTREAM_CNOT) {                                    // (fa != fb; no word, no flags)
                    if (MODE == MS_STORE || alive) {
                        Tb ^= Ta & MS_LOW;
                        Ta ^= Tb & MS_HIGH;
                        Ta ^= l, Tb ^= t;
#pragma unroll
                        for (int q = 0; q < NF; ++q) {
                            if (q == fa) T[q] = Ta;
                            if (q == fb) T[q] = Tb;
                        }
                        if constexpr (MODE == MS_TALLY) {
                            if (a.propagated) {
                                u64 Ra = 0, Rb = 0;
#pragma unroll
                                for (int q = 0; q < NF; ++q) {
                                    if (q == fa) Ra = R[q];
                                    if (q == fb) Rb = R[q];
                                }
                                Rb ^= Ra & MS_LOW;
                                Ra ^= Rb & MS_HIGH;
#pragma unroll
                                for (int q = 0; q < NF; ++q) {
                                    if (q == fa) R[q] = Ra;
                                    if (q == fb) R[q] = Rb;
                                }
                            }
                        }
                    }
                } else {
                    const u64 frame = kind == GF2_STREAM_EC ? ~(1ull << 31 | 1ull << 63) : kind == GF2_STREAM_MEASURE ? MS_LOW : 0ull;
                    const u64 word = (Ta & frame) ^ l;
                    if constexpr (MODE == MS_STORE) {
                        if (info.y >= 0) row[info.y] = word;
                        if (f) {
                            u64* fw = row + a.nsteps + (info.z >> 6);
                            const int sh = info.z & 63;
                            fw[0] |= f << sh;
                            if (sh && (f >> (64 - sh))) fw[1] |= f >> (64 - sh);   // (a bit below the type's flag rows: the word exists)
                        }
                        Ta ^= t;
                    } else if (alive) {
                        if (f) {
                            alive = false;                                         // a verification fired: the sample is rejected
                        } else {
                            if (kind != GF2_STREAM_NONE) {
                                u64 Ra = 0;
#pragma unroll
                                for (int q = 0; q < NF; ++q)
                                    if (q == fa) Ra = R[q];
#pragma unroll
                                for (int c = 0; c < 2; ++c) {
                                    if (c == 0 || kind == GF2_STREAM_EC) {         // a measurement corrects data.x_errors only
                                        const u64 v = ((word ^ Ra) >> (32 * c)) & a.mask[c];
                                        if (v != 0 || !a.zero_ok[c]) {             // (v = 0 and zero_ok: found, K ^= 0, P ^= 0)
                                            const u64 hit = hash_find<1>(a.tab[c], 0ull, v);
                                            if (hit == ~0ull)
                                                unmatched[c] += 1;                 // css_code.py:655-657: no match, nothing recorded
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
                            Ta ^= t;
                        }
                    }
#pragma unroll
                    for (int q = 0; q < NF; ++q)
                        if (q == fa) T[q] = Ta;
                }
                closed += 1;
            }
            if (closed) {                                                          // the block that goes on, if any, moves to slot 0
                u64 l = 0, t = 0, f = 0;
#pragma unroll
                for (int j = 1; j < MS_NACC; ++j)
                    if (j == closed) l = acc_l[j], t = acc_t[j], f = acc_f[j];
#pragma unroll
                for (int j = 1; j < MS_NACC; ++j) acc_l[j] = acc_t[j] = acc_f[j] = 0;
                acc_l[0] = l, acc_t[0] = t, acc_f[0] = f;
                lo += closed;
            }
        }
        if constexpr (MODE == MS_TALLY) {
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
            }
        }
    }
    if constexpr (MODE == MS_TALLY) {
        if (accepted) atomicAdd(&bins[0], accepted);
        __syncthreads();
        if (threadIdx.x < MS_FIELDS && bins[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (u64)bins[threadIdx.x]);
    }
}

// A lane adds at most nsteps to a field per sample (unmatched keys, wrong trials), a workgroup's 32-bit LDS bins hold the sum over
// its 256 lanes: with at most `per_lane` samples per lane, 256 * per_lane * nsteps must stay below 2^32 (gf2_stream.hip's rule).
static int64_t ms_per_lane_cap(int64_t nsteps) { return (int64_t)(0xFFFFFFFFll / (256 * (nsteps > 1 ? nsteps : 1))); }

template <int MODE, int NF>
static int mstream_launch_frames(gf2_ctx* ctx, const gf2_mstream* ms, const MStreamArgs& a) {
    const size_t eff_bytes = (size_t)ms->table_words * 8;
    const size_t base = (size_t)2 * GF2_SEG_CDF * 8 + (size_t)CIRC_THREADS * CIRC_TAKEN_STRIDE * 4 + 32 * 4;
    const bool staged = base + eff_bytes <= MS_LDS_MAX;
    const size_t lds = base + (staged ? eff_bytes : 0);
    // samples per lane: a long program is many segments per sample, so fewer samples per lane keep the grid wide
    int64_t per_lane = 64 / a.th.nseg;
    if (per_lane > 16) per_lane = 16;
    if (per_lane < 1) per_lane = 1;
    const int64_t cap = ms_per_lane_cap(ms->plan.seq.nsteps);
    if (per_lane > cap) per_lane = cap;
    int64_t blocks = gf2_cdiv(a.count, CIRC_THREADS * per_lane);
    // (the tally keeps count <= MS_MAX_BLOCKS * 256 * cap for its LDS bins; the store, which has no bins, MS_MAX_BLOCKS * 256 * 16)
    if (blocks > MS_MAX_BLOCKS) blocks = MS_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    if (staged && lds > 64 * 1024)
        GF2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mstream_kernel<MODE, true, NF>), hipFuncAttributeMaxDynamicSharedMemorySize, MS_LDS_MAX));
    GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
    if (staged)
        hipLaunchKernelGGL((mstream_kernel<MODE, true, NF>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    else
        hipLaunchKernelGGL((mstream_kernel<MODE, false, NF>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    GF2_TRY(gf2_prof_end(ctx));
    GF2_HIP(hipGetLastError());
    return GF2_OK;
}

template <int MODE>
static int mstream_launch(gf2_ctx* ctx, const gf2_mstream* ms, const MStreamArgs& a) {
    const int64_t nframes = ms->plan.nframes;
    if (nframes == 1) return mstream_launch_frames<MODE, 1>(ctx, ms, a);
    if (nframes == 2) return mstream_launch_frames<MODE, 2>(ctx, ms, a);
    return mstream_launch_frames<MODE, 4>(ctx, ms, a);
}

static void mstream_args(const gf2_mstream* ms, uint64_t seed, MStreamArgs* a) {
    a->eff = ms->eff_dev;
    a->eff_words = (int)ms->table_words;
    a->seed = seed;
    a->start = ms->start_dev;
    a->delta = ms->delta_dev;
    a->info = ms->info_dev;
    a->nblocks = (int)ms->nblocks;
    a->locations = (int)ms->plan.seq.locations;
    a->nsteps = (int)ms->plan.seq.nsteps;
    a->flag_words = (int)ms->plan.seq.flag_words;
    a->trials = (int)ms->plan.seq.trials;
    a->measurements = (int)ms->plan.measurements;
}

extern "C" {

int gf2_mstream_destroy(gf2_ctx* ctx, gf2_mstream* mstream) {
    if (!ctx) GF2_FAIL(GF2_E_ARG, "gf2_mstream_destroy: null context");
    if (!mstream) return GF2_OK;
    GF2_TRY(gf2_ctx_activate(ctx));
    (void)gf2_dev_free(ctx, mstream->eff_dev);
    (void)gf2_dev_free(ctx, mstream->start_dev);
    (void)gf2_dev_free(ctx, mstream->delta_dev);
    (void)gf2_dev_free(ctx, mstream->info_dev);
    delete mstream;
    return GF2_OK;
}

int gf2_mstream_create(gf2_ctx* ctx, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                       const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                       int64_t nframes, gf2_mstream** mstream_out) {
    const char* who = "gf2_mstream_create";
    if (!ctx || !mstream_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    *mstream_out = nullptr;
    gf2_mstream* ms = new (std::nothrow) gf2_mstream();
    if (!ms) GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    ms->eff_dev = nullptr, ms->start_dev = nullptr, ms->delta_dev = nullptr, ms->info_dev = nullptr;
    int rc = gf2_mstream_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, block_a, block_b, nblocks, nframes, &ms->plan);
    if (rc == GF2_OK) rc = gf2_mstream_check_overlap(who, ms->plan, nblocks);
    if (rc != GF2_OK) {
        delete ms;
        return rc;
    }
    const StreamPlan& plan = ms->plan.seq;
    ms->nblocks = nblocks;
    int64_t rows = 0;
    for (int64_t t = 0; t < ntypes; ++t) rows += type_locations[t];
    ms->table_words = rows * 6;
    std::vector<int> start, delta;
    std::vector<int4> info;
    try {
        start.assign((size_t)nblocks + 2 + MS_NACC, INT_MAX);
        delta.assign((size_t)nblocks + MS_NACC, 0);
        info.resize((size_t)nblocks);
    } catch (const std::bad_alloc&) {
        delete ms;
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    for (int64_t b = 0; b < nblocks; ++b) {
        start[(size_t)b] = plan.start[(size_t)b];
        const int kind = block_kind[b];
        delta[(size_t)b] = (int)(plan.type_offset[(size_t)block_type[b]] - plan.start[(size_t)b]);
        const int fb = kind == GF2_MSTREAM_CNOT ? block_b[b] : block_a[b];
        const int m = ms->plan.measure[(size_t)b] < 0 ? 0 : ms->plan.measure[(size_t)b];
        info[(size_t)b] = make_int4(kind | (ms->plan.first_trial[(size_t)b] ? 8 : 0) | block_a[b] << 4 | fb << 6 | m << 8, plan.step[(size_t)b],
                                    plan.flag[(size_t)b], 0);
    }
    start[(size_t)nblocks] = (int)plan.locations;
    rc = gf2_ctx_activate(ctx);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, (size_t)ms->table_words * 8, (void**)&ms->eff_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, start.size() * 4, (void**)&ms->start_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, delta.size() * 4, (void**)&ms->delta_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, info.size() * 16, (void**)&ms->info_dev);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, ms->eff_dev, type_eff, (size_t)ms->table_words * 8);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, ms->start_dev, start.data(), start.size() * 4);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, ms->delta_dev, delta.data(), delta.size() * 4);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, ms->info_dev, info.data(), info.size() * 16);
    if (rc != GF2_OK) {
        (void)gf2_mstream_destroy(ctx, ms);
        return rc;
    }
    *mstream_out = ms;
    return GF2_OK;
}

int gf2_mstream_outcomes_dev(gf2_ctx* ctx, const gf2_mstream* mstream, uint64_t seed, int64_t first_sample, int64_t count, double p_x,
                             double p_y, double p_z, uint64_t* out_dev, int64_t ldo) {
    const char* who = "gf2_mstream_outcomes_dev";
    if (!ctx || !mstream) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "%s: negative range", who);
    const int64_t ldr = mstream->plan.seq.nsteps + mstream->plan.seq.flag_words;
    if (ldo < ldr) GF2_FAIL(GF2_E_ARG, "%s: ldo must be at least the sequence's nsteps + F = %lld words", who, (long long)ldr);
    GF2_TRY(check_probabilities(p_x, p_y, p_z));
    if (count == 0) return GF2_OK;
    if (!out_dev) GF2_FAIL(GF2_E_ARG, "%s: null buffer", who);
    GF2_TRY(gf2_ctx_activate(ctx));
    MStreamArgs a = {};
    GF2_TRY(gf2_seg_tables(ctx, p_x, p_y, p_z, mstream->plan.seq.locations, &a.th));
    mstream_args(mstream, seed, &a);
    a.ldo = ldo;
    const int64_t most = (int64_t)MS_MAX_BLOCKS * CIRC_THREADS * 16;
    for (int64_t done = 0; done < count; done += most) {
        a.first_sample = first_sample + done;
        a.count = count - done < most ? count - done : most;
        a.out = (u64*)out_dev + done * ldo;
        GF2_TRY((mstream_launch<MS_STORE>(ctx, mstream, a)));
    }
    return GF2_OK;
}

int gf2_mc_mstream_decode(gf2_ctx* ctx, const gf2_mstream* mstream, int64_t records, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                          int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed,
                          int64_t first_sample, int64_t count, double p_x, double p_y, double p_z, uint64_t* counts_out) {
    const char* who = "gf2_mc_mstream_decode";
    if (!ctx || !mstream || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GF2_TRY(gf2_mstream_check_records(who, records));
    GF2_TRY(gf2_mstream_check_bits(who, mstream->plan, r1, r2));
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "%s: negative range", who);
    GF2_TRY(check_probabilities(p_x, p_y, p_z));
    GF2_TRY(gf2_ctx_activate(ctx));
    for (int k = 0; k < MS_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    MStreamArgs a = {};
    GF2_TRY(gf2_seg_tables(ctx, p_x, p_y, p_z, mstream->plan.seq.locations, &a.th));
    mstream_args(mstream, seed, &a);
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
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, MS_FIELDS, &a));
    a.counts = tables.counts_dev;
    const int64_t most = (int64_t)MS_MAX_BLOCKS * CIRC_THREADS * ms_per_lane_cap(mstream->plan.seq.nsteps);
    for (int64_t done = 0; done < count; done += most) {
        a.first_sample = first_sample + done;
        a.count = count - done < most ? count - done : most;
        GF2_TRY((mstream_launch<MS_TALLY>(ctx, mstream, a)));
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, MS_FIELDS * 8);
}

}  // extern "C"
