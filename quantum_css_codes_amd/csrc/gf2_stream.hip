// Streamed gadgets (DESIGN.md "Streamed gadgets", include/gf2hip.h): error-correction cycles and rewritten programs of any length,
// walked block by block.  gf2_ec.hip and gf2_ft.hip hold a sample's outcome words in registers and gather from one dense effect table
// of 2 L ldr words, which caps them at 6 rounds / 16 words.  Here a gadget is a sequence of blocks of a handful of types, a fault acts
// through three words -- (local, tail, flags) of its own block -- and the data frame T carries everything from one block to the next,
// so memory and work per sample are linear in the number of blocks.
//
// Lane = sample.  The sampler is circuit_gather's, draw for draw (sample_key, segment_draw, error_count, error_draw, Floyd's rule
// over all L locations in 512-location segments), so sample i has the faults it has in the resident kernels.  Segments ascend in
// time but the faults of one segment come in Floyd's order, and a segment overlaps up to GF2_STREAM_MAX_OVERLAP blocks: a lane keeps
// one (local, tail, flags) accumulator per overlapped block, slot j for block lo + j, lo = the first block not yet closed (uniform
// across the grid: it depends on the segment alone).  After a segment's faults the blocks that end in it are closed in order, also
// when the segment drew no fault:
//     word = mask_kind(T) ^ local;  a non-zero flags rejects the sample, before any lookup;  the step's lookups;  T ^= tail
// and the accumulator of the one block that goes on into the next segment moves to slot 0.  The accumulators never take a run-time
// index: a fault finds its slot by a chain of compares against the blocks' first locations (uniform, scalar registers) and is
// added through a chain of selects; the block being closed is picked through another (gf2_ec.hip's header says why: a run-time
// index would put the arrays into scratch).  The kernels use no scratch (DESIGN.md has the build's figures).
//
// Tally: the rules of gf2_ec.hip and gf2_ft.hip word for word -- one record (K, P) per side, an EC step updates both, a MEASURE step
// the x side only, the FINAL step judges T.  A lookup of the key v = 0 is skipped when the host has found the zero key in the
// side's table with flip 0 (zero_ok): finding it would change neither K nor P.  That is the whole of a fault-free block while
// T = K = 0.  A rejected lane leaves its sample's walk at once; its wavefront goes on for the others.
//
// LDS per workgroup: the sampler's two inverse-CDF tables, the taken maps, the twelve counts, and the block types' tables when all
// of that fits 160 KiB (the Steane cycle: 16 KB; all seven Steane types: 78 KB); otherwise the tables are read through L2.
#include <limits.h>

#include <new>
#include <vector>

#include "gf2_internal.h"
#include "gf2_circuit_dev.h"
#include "gf2_stream_plan.h"

#define ST_NACC GF2_STREAM_MAX_OVERLAP
#define ST_FIELDS GF2_STREAM_FIELDS
#define ST_LDS_MAX (160 * 1024)
#define ST_MAX_BLOCKS 4096
#define ST_FIRST_MEASURE 4                     // bit of StreamArgs::info[b].x beside the kind

enum { ST_STORE = 0, ST_TALLY = 1 };

struct gf2_stream {
    StreamPlan plan;
    int64_t nblocks, table_words;              // blocks, the FINAL step included; words of all types' tables
    u64* eff_dev;
    int* start_dev;                            // nblocks + 1 first locations (the last: L), then ST_NACC + 1 times INT_MAX
    int* delta_dev;                            // nblocks + ST_NACC: the type's first table row - the block's first location (pads 0)
    int4* info_dev;                            // nblocks: (kind | ST_FIRST_MEASURE, step or -1, first flag row, 0)
};

struct StreamArgs {
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
    int trials;
    u64 mask[2];                               // [0]: the r_2 bits of key_x, [1]: the r_1 bits of key_z
    int kwx, kwz;                              // 1 and 1 (CircuitTables reads them)
    HashTab tab[2];                            // [0]: parity_check_c2's table (key_x), [1]: parity_check_c1's (key_z)
    const unsigned char* flips[2];             // operator . correction of every table entry
    int zero_ok[2];                            // the side's table holds the key 0 with flip 0
    u64* counts;
};

template <int MODE, bool STAGED>
__global__ __launch_bounds__(CIRC_THREADS) void stream_kernel(StreamArgs a) {
    extern __shared__ u64 st_lds[];
    u64* cdf_lds = st_lds;                                                         // [2][GF2_SEG_CDF]
    u64* eff_lds = st_lds + 2 * GF2_SEG_CDF;
    unsigned int* taken = (unsigned int*)(eff_lds + (STAGED ? a.eff_words : 0));
    unsigned int* bins = taken + CIRC_THREADS * CIRC_TAKEN_STRIDE;                 // ST_FIELDS
    for (int i = threadIdx.x; i < 2 * GF2_SEG_CDF; i += blockDim.x)
        if (a.th.nseg > 1 || i >= GF2_SEG_CDF) cdf_lds[i] = a.th.cdf[i];            // (one segment: only the last one's table is read)
    if (STAGED)
        for (int i = threadIdx.x; i < a.eff_words; i += blockDim.x) eff_lds[i] = a.eff[i];
    if (MODE == ST_TALLY && threadIdx.x < ST_FIELDS) bins[threadIdx.x] = 0;
    __syncthreads();
    const u64* eff = STAGED ? eff_lds : a.eff;
    unsigned int* mine = taken + threadIdx.x * CIRC_TAKEN_STRIDE;
    unsigned int local[ST_FIELDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += stride) {
        const u64 ks = sample_key(a.seed, (u64)(a.first_sample + i));
        u64 T = 0, K[2] = {0, 0};                                                  // the data frame; syndrome of the errors recorded so far, per side
        unsigned int P[2] = {0, 0}, unmatched[2] = {0, 0};                         // ... and their operator parity
        unsigned int wrong_trials = 0, first_wrong = 0, final_bits = 0;           // final_bits: flip_x, flip_z, miss_x, miss_z
        u64 acc_l[ST_NACC], acc_t[ST_NACC], acc_f[ST_NACC];                        // slot j: block lo + j
#pragma unroll
        for (int j = 0; j < ST_NACC; ++j) acc_l[j] = acc_t[j] = acc_f[j] = 0;
        u64* row = MODE == ST_STORE ? a.out + i * a.ldo : nullptr;
        if constexpr (MODE == ST_STORE)
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
                int st[ST_NACC], dl[ST_NACC];                                      // uniform: constant indices only
#pragma unroll
                for (int j = 0; j < ST_NACC; ++j) st[j] = a.start[lo + j], dl[j] = a.delta[lo + j];
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
                    for (int j = 1; j < ST_NACC; ++j)
                        if (g >= st[j]) slot = j, base = dl[j];                    // (the pads are INT_MAX: never taken)
                    const u64* e = eff + (size_t)(base + g) * 6;
                    u64 vl = 0, vt = 0, vf = 0;
                    if (kind & 1u) vl ^= e[0], vt ^= e[1], vf ^= e[2];
                    if (kind & 2u) vl ^= e[3], vt ^= e[4], vf ^= e[5];
#pragma unroll
                    for (int j = 0; j < ST_NACC; ++j)
                        if (slot == j) acc_l[j] ^= vl, acc_t[j] ^= vt, acc_f[j] ^= vf;
                }
            }
            // close the blocks that end in this segment, in order (all of it uniform but the lanes' own words)
            int closed = 0;
#pragma unroll 1
            while (closed < ST_NACC && lo + closed < a.nblocks && a.start[lo + closed + 1] <= seg_end) {
                u64 l = 0, t = 0, f = 0;
#pragma unroll
                for (int j = 0; j < ST_NACC; ++j)
                    if (j == closed) l = acc_l[j], t = acc_t[j], f = acc_f[j];
                const int4 info = a.info[lo + closed];
                const int kind = info.x & 3;
                const u64 frame = kind == GF2_STREAM_EC ? ~(1ull << 31 | 1ull << 63) : kind == GF2_STREAM_MEASURE ? 0xFFFFFFFFull : kind == GF2_STREAM_FINAL ? ~0ull : 0ull;
                const u64 word = (T & frame) ^ l;
                if constexpr (MODE == ST_STORE) {
                    if (info.y >= 0) row[info.y] = word;
                    if (f) {
                        u64* fw = row + a.nsteps + (info.z >> 6);
                        const int sh = info.z & 63;
                        fw[0] |= f << sh;
                        if (sh && (f >> (64 - sh))) fw[1] |= f >> (64 - sh);       // (a bit below the type's flag rows: the word exists)
                    }
                    T ^= t;
                } else if (alive) {
                    if (f) {
                        alive = false;                                             // a verification fired: the attempt is repeated
                    } else {
                        if (kind == GF2_STREAM_EC || kind == GF2_STREAM_MEASURE) {
#pragma unroll
                            for (int c = 0; c < 2; ++c) {
                                if (c == 0 || kind == GF2_STREAM_EC) {             // a measurement corrects data.x_errors only
                                    const u64 v = ((word >> (32 * c)) & a.mask[c]) ^ K[c];
                                    if (v != 0 || !a.zero_ok[c]) {                 // (v = 0 and zero_ok: found, K ^= 0, P ^= 0)
                                        const u64 hit = hash_find<1>(a.tab[c], 0ull, v);
                                        if (hit == ~0ull) {
                                            unmatched[c] += 1;                     // css_code.py:655-657: no match, nothing recorded
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
                                if (info.x & ST_FIRST_MEASURE) first_wrong = bad;
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
                        T ^= t;
                    }
                }
                closed += 1;
            }
            if (closed) {                                                          // the block that goes on, if any, moves to slot 0
                u64 l = 0, t = 0, f = 0;
#pragma unroll
                for (int j = 1; j < ST_NACC; ++j)
                    if (j == closed) l = acc_l[j], t = acc_t[j], f = acc_f[j];
#pragma unroll
                for (int j = 1; j < ST_NACC; ++j) acc_l[j] = acc_t[j] = acc_f[j] = 0;
                acc_l[0] = l, acc_t[0] = t, acc_f[0] = f;
                lo += closed;
            }
        }
        if constexpr (MODE == ST_TALLY) {
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
            }
        }
    }
    if constexpr (MODE == ST_TALLY) {
#pragma unroll
        for (int k = 0; k < ST_FIELDS; ++k)
            if (local[k]) atomicAdd(&bins[k], local[k]);
        __syncthreads();
        if (threadIdx.x < ST_FIELDS && bins[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (u64)bins[threadIdx.x]);
    }
}

// A lane adds at most nsteps to a field per sample (unmatched keys, wrong trials), a workgroup's 32-bit LDS bins hold the sum over
// its 256 lanes: with at most `per_lane` samples per lane, 256 * per_lane * nsteps must stay below 2^32.  st_per_lane_cap is the
// largest such per_lane (nsteps <= 2^20 + 1: at least 15); a launch takes at most ST_MAX_BLOCKS * 256 * cap samples and spreads
// them over enough workgroups that no lane gets more than cap.
static int64_t st_per_lane_cap(int64_t nsteps) { return (int64_t)(0xFFFFFFFFll / (256 * (nsteps > 1 ? nsteps : 1))); }

template <int MODE>
static int stream_launch(gf2_ctx* ctx, const gf2_stream* st, const StreamArgs& a) {
    const size_t eff_bytes = (size_t)st->table_words * 8;
    const size_t base = (size_t)2 * GF2_SEG_CDF * 8 + (size_t)CIRC_THREADS * CIRC_TAKEN_STRIDE * 4 + 16 * 4;
    const bool staged = base + eff_bytes <= ST_LDS_MAX;
    const size_t lds = base + (staged ? eff_bytes : 0);
    // samples per lane: a long gadget is many segments per sample, so fewer samples per lane keep the grid wide
    int64_t per_lane = 64 / a.th.nseg;
    if (per_lane > 16) per_lane = 16;
    if (per_lane < 1) per_lane = 1;
    const int64_t cap = st_per_lane_cap(st->plan.nsteps);
    if (per_lane > cap) per_lane = cap;
    int64_t blocks = gf2_cdiv(a.count, CIRC_THREADS * per_lane);
    if (blocks > ST_MAX_BLOCKS) blocks = ST_MAX_BLOCKS;                             // (the caller keeps count <= ST_MAX_BLOCKS * 256 * cap)
    if (blocks < 1) blocks = 1;
    if (staged && lds > 64 * 1024)
        GF2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(stream_kernel<MODE, true>), hipFuncAttributeMaxDynamicSharedMemorySize, ST_LDS_MAX));
    GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
    if (staged)
        hipLaunchKernelGGL((stream_kernel<MODE, true>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    else
        hipLaunchKernelGGL((stream_kernel<MODE, false>), dim3((unsigned)blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    GF2_TRY(gf2_prof_end(ctx));
    GF2_HIP(hipGetLastError());
    return GF2_OK;
}

static void stream_args(const gf2_stream* st, uint64_t seed, StreamArgs* a) {
    a->eff = st->eff_dev;
    a->eff_words = (int)st->table_words;
    a->seed = seed;
    a->start = st->start_dev;
    a->delta = st->delta_dev;
    a->info = st->info_dev;
    a->nblocks = (int)st->nblocks;
    a->locations = (int)st->plan.locations;
    a->nsteps = (int)st->plan.nsteps;
    a->flag_words = (int)st->plan.flag_words;
    a->trials = (int)st->plan.trials;
}

extern "C" {

int gf2_stream_destroy(gf2_ctx* ctx, gf2_stream* stream) {
    if (!ctx) GF2_FAIL(GF2_E_ARG, "gf2_stream_destroy: null context");
    if (!stream) return GF2_OK;
    GF2_TRY(gf2_ctx_activate(ctx));
    (void)gf2_dev_free(ctx, stream->eff_dev);
    (void)gf2_dev_free(ctx, stream->start_dev);
    (void)gf2_dev_free(ctx, stream->delta_dev);
    (void)gf2_dev_free(ctx, stream->info_dev);
    delete stream;
    return GF2_OK;
}

int gf2_stream_create(gf2_ctx* ctx, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                      const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, gf2_stream** stream_out) {
    const char* who = "gf2_stream_create";
    if (!ctx || !stream_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    *stream_out = nullptr;
    gf2_stream* st = new (std::nothrow) gf2_stream();
    if (!st) GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    st->eff_dev = nullptr, st->start_dev = nullptr, st->delta_dev = nullptr, st->info_dev = nullptr;
    int rc = gf2_stream_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, nblocks, &st->plan);
    if (rc != GF2_OK) {
        delete st;
        return rc;
    }
    const StreamPlan& plan = st->plan;
    // the blocks a segment overlaps: those with a location in it, and the FINAL step with the last segment
    for (int64_t seg = 0, lo = 0; seg * GF2_SEG_BITS < plan.locations; ++seg) {
        const int64_t seg_start = seg * GF2_SEG_BITS, seg_end = seg_start + GF2_SEG_BITS < plan.locations ? seg_start + GF2_SEG_BITS : plan.locations;
        while (plan.start[(size_t)lo + 1] <= seg_start) lo += 1;
        int64_t hi = lo;
        while (hi + 1 < nblocks && plan.start[(size_t)hi + 1] < seg_end) hi += 1;
        if (seg_end == plan.locations) hi = nblocks - 1;
        if (hi - lo + 1 > ST_NACC) {
            delete st;
            GF2_FAIL(GF2_E_ARG, "%s: locations %lld .. %lld (one 512-location segment of the sampler) overlap %lld blocks, more than %d", who,
                     (long long)seg_start, (long long)seg_end - 1, (long long)(hi - lo + 1), ST_NACC);
        }
    }
    st->nblocks = nblocks;
    int64_t rows = 0;
    for (int64_t t = 0; t < ntypes; ++t) rows += type_locations[t];
    st->table_words = rows * 6;
    std::vector<int> start, delta;
    std::vector<int4> info;
    try {
        start.assign((size_t)nblocks + 2 + ST_NACC, INT_MAX);
        delta.assign((size_t)nblocks + ST_NACC, 0);
        info.resize((size_t)nblocks);
    } catch (const std::bad_alloc&) {
        delete st;
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    bool seen_measure = false;
    for (int64_t b = 0; b < nblocks; ++b) {
        start[(size_t)b] = plan.start[(size_t)b];
        const int kind = block_kind[b];
        if (kind != GF2_STREAM_FINAL) delta[(size_t)b] = (int)(plan.type_offset[(size_t)block_type[b]] - plan.start[(size_t)b]);
        info[(size_t)b] = make_int4(kind | (kind == GF2_STREAM_MEASURE && !seen_measure ? ST_FIRST_MEASURE : 0), plan.step[(size_t)b], plan.flag[(size_t)b], 0);
        seen_measure |= kind == GF2_STREAM_MEASURE;
    }
    start[(size_t)nblocks] = (int)plan.locations;
    rc = gf2_ctx_activate(ctx);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, (size_t)st->table_words * 8, (void**)&st->eff_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, start.size() * 4, (void**)&st->start_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, delta.size() * 4, (void**)&st->delta_dev);
    if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, info.size() * 16, (void**)&st->info_dev);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, st->eff_dev, type_eff, (size_t)st->table_words * 8);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, st->start_dev, start.data(), start.size() * 4);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, st->delta_dev, delta.data(), delta.size() * 4);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, st->info_dev, info.data(), info.size() * 16);
    if (rc != GF2_OK) {
        (void)gf2_stream_destroy(ctx, st);
        return rc;
    }
    *stream_out = st;
    return GF2_OK;
}

int gf2_stream_outcomes_dev(gf2_ctx* ctx, const gf2_stream* stream, uint64_t seed, int64_t first_sample, int64_t count, double p_x,
                            double p_y, double p_z, uint64_t* out_dev, int64_t ldo) {
    const char* who = "gf2_stream_outcomes_dev";
    if (!ctx || !stream) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "%s: negative range", who);
    const int64_t ldr = stream->plan.nsteps + stream->plan.flag_words;
    if (ldo < ldr) GF2_FAIL(GF2_E_ARG, "%s: ldo must be at least the sequence's nsteps + F = %lld words", who, (long long)ldr);
    GF2_TRY(check_probabilities(p_x, p_y, p_z));
    if (count == 0) return GF2_OK;
    if (!out_dev) GF2_FAIL(GF2_E_ARG, "%s: null buffer", who);
    GF2_TRY(gf2_ctx_activate(ctx));
    StreamArgs a = {};
    GF2_TRY(gf2_seg_tables(ctx, p_x, p_y, p_z, stream->plan.locations, &a.th));
    stream_args(stream, seed, &a);
    a.ldo = ldo;
    const int64_t most = (int64_t)ST_MAX_BLOCKS * CIRC_THREADS * 16;
    for (int64_t done = 0; done < count; done += most) {
        a.first_sample = first_sample + done;
        a.count = count - done < most ? count - done : most;
        a.out = (u64*)out_dev + done * ldo;
        GF2_TRY((stream_launch<ST_STORE>(ctx, stream, a)));
    }
    return GF2_OK;
}

int gf2_mc_stream_decode(gf2_ctx* ctx, const gf2_stream* stream, int64_t r1, const uint64_t* keys1, const uint8_t* flips1, int64_t entries1,
                         int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed, int64_t first_sample,
                         int64_t count, double p_x, double p_y, double p_z, uint64_t* counts_out) {
    const char* who = "gf2_mc_stream_decode";
    if (!ctx || !stream || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GF2_TRY(gf2_stream_check_bits(who, stream->plan, r1, r2));
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "%s: negative range", who);
    GF2_TRY(check_probabilities(p_x, p_y, p_z));
    GF2_TRY(gf2_ctx_activate(ctx));
    for (int k = 0; k < ST_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    StreamArgs a = {};
    GF2_TRY(gf2_seg_tables(ctx, p_x, p_y, p_z, stream->plan.locations, &a.th));
    stream_args(stream, seed, &a);
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
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, ST_FIELDS, &a));
    a.counts = tables.counts_dev;
    const int64_t most = (int64_t)ST_MAX_BLOCKS * CIRC_THREADS * st_per_lane_cap(stream->plan.nsteps);
    for (int64_t done = 0; done < count; done += most) {
        a.first_sample = first_sample + done;
        a.count = count - done < most ? count - done : most;
        GF2_TRY((stream_launch<ST_TALLY>(ctx, stream, a)));
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, ST_FIELDS * 8);
}

}  // extern "C"
