// What the kernels over a circuit's effect table share -- gf2_circuit.hip (the fault Monte-Carlo), gf2_enumerate.hip (the exact
// strata), gf2_stream.hip (the streamed route) and the entry points of the two post-selected gadgets: gf2_ec.hip (the
// error-correction cycle), gf2_ft.hip (the fault-tolerant logical measurement), gf2_gadget_strata.hip (their sampled strata),
// gf2_gadget_enumerate.hip (their exact strata), gf2_gate_enumerate.hip (those under gate-level faults), gf2_gadget_list.hip and gf2_gate_list.hip
// (their malignant fault sets): the circuit object, the Monte-Carlo layout of its outcome words, whether a launch stages the effect
// table in LDS, the device side of the tally's syndrome tables and the gather loop of a Monte-Carlo sample.
#pragma once

#include "gf2_internal.h"
#include "gf2_hash_dev.h"
#include "gf2_sampler.h"

#define CIRC_THREADS 256
#define CIRC_EFF_LDS_BYTES 20480               // effect tables up to this size are staged in LDS
#define CIRC_TAKEN_STRIDE 17                   // dwords per lane: 16 hold the 512 bits

struct gf2_circuit {
    int64_t locations, ldr;
    u64* eff_dev;                              // 2 * locations * ldr words
    u64 any[GF2_FT_MAX_LDR];                   // OR of all effects, word by word: which outcome bits can be set at all
};

// gf2_circuit.hip: gf2_circuit_create for 1 <= ldr <= max_ldr (gf2_ft_circuit_create's GF2_FT_MAX_LDR: gf2_ft.hip)
int gf2_circuit_create_upto(const char* who, gf2_ctx* ctx, const uint64_t* eff, int64_t locations, int64_t ldr, int64_t max_ldr,
                            gf2_circuit** circuit_out);

// Whether a launch stages the circuit's effect table in LDS (allowed: the kernel has a staged form; the table must fit
// CIRC_EFF_LDS_BYTES), and the launch's dynamic LDS: the staged table plus `other` bytes.
static bool circuit_staged(const gf2_circuit* circ, bool allowed, size_t other, size_t* lds) {
    const size_t eff_bytes = (size_t)2 * circ->locations * circ->ldr * 8;
    const bool staged = allowed && eff_bytes <= CIRC_EFF_LDS_BYTES;
    *lds = (staged ? eff_bytes : 0) + other;
    return staged;
}

// gf2_host.cpp: the argument rules of an enumerated rank range (include/gf2hip.h "exact strata")
int gf2_enum_check_range(const char* who, int64_t nb, int64_t w, int64_t first_rank, int64_t count);

// The Monte-Carlo layout of a circuit's words for checks of r_1 and r_2 rows, tested against what the table can set.  Args: a
// kernel's argument block with kwx and kwz.
template <class Args>
static int circuit_layout(const char* who, const gf2_circuit* circ, int64_t r1, int64_t r2, Args* a) {
    if (r1 < 1 || r2 < 1 || r1 > 127 || r2 > 127) GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= r_1, r_2 <= 127", who);
    a->kwx = r2 <= 63 ? 1 : 2;
    a->kwz = r1 <= 63 ? 1 : 2;
    if (circ->ldr != a->kwx + a->kwz + 1)
        GF2_FAIL(GF2_E_ARG, "%s: r_1 = %lld and r_2 = %lld need effects of %d words (key_x, key_z, parity), the circuit has %lld", who,
                 (long long)r1, (long long)r2, a->kwx + a->kwz + 1, (long long)circ->ldr);
    auto beyond = [](const u64* words, int kw, int64_t r) {            // a bit at or above r in a key of kw words
        const int64_t top = r - 64 * (kw - 1);                           // bits of the highest word (1 .. 63)
        return (words[kw - 1] >> top) != 0;
    };
    if (beyond(circ->any, a->kwx, r2) || beyond(circ->any + a->kwx, a->kwz, r1) || (circ->any[circ->ldr - 1] >> 2) != 0)
        GF2_FAIL(GF2_E_ARG, "%s: the effects set bits beyond the keys' r_2 / r_1 bits or the two parity bits", who);
    return GF2_OK;
}

static int circuit_check_tables(const char* who, const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, const uint64_t* keys2,
                                const uint8_t* flips2, int64_t entries2) {
    if (entries1 < 0 || entries2 < 0 || (entries1 && (!keys1 || !flips1)) || (entries2 && (!keys2 || !flips2)))
        GF2_FAIL(GF2_E_ARG, "%s: bad table (a null array with entries > 0, or a negative count)", who);
    if (entries1 > (int64_t)TBL_HASH_MAX_ENTRIES || entries2 > (int64_t)TBL_HASH_MAX_ENTRIES) GF2_FAIL(GF2_E_ARG, "%s: table too large", who);
    return GF2_OK;
}

// The device side of the tally's tables (a.kwx and a.kwz set): keys in hash tables, one flip byte per entry, zeroed counts.
// Side 0: key_x against parity_check_c2's table; side 1: key_z against parity_check_c1's.  Freed with the object.
struct CircuitTables {
    gf2_ctx* ctx;
    HashAlloc tabs[2];
    void* dev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    u64* counts_dev = nullptr;
    int* flags_dev = nullptr;
    explicit CircuitTables(gf2_ctx* c) : ctx(c), tabs{HashAlloc(c), HashAlloc(c)} {}
    ~CircuitTables() {
        for (int c = 0; c < 2; ++c)
            for (int k = 0; k < 2; ++k) (void)gf2_dev_free(ctx, dev[c][k]);
        (void)gf2_dev_free(ctx, flags_dev);
        (void)gf2_dev_free(ctx, counts_dev);
    }
    template <class Args>
    int make(const char* who, const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, const uint64_t* keys2, const uint8_t* flips2,
             int64_t entries2, int64_t ncounts, Args* a) {
        const int64_t es[2] = {entries2, entries1};
        const uint64_t* ks[2] = {keys2, keys1};
        const uint8_t* fs[2] = {flips2, flips1};
        const int kws[2] = {a->kwx, a->kwz};
        int rc = gf2_dev_alloc(ctx, 16, (void**)&flags_dev);
        if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, (size_t)ncounts * 8, (void**)&counts_dev);
        if (rc == GF2_OK && (hipMemsetAsync(flags_dev, 0, 16, ctx->stream) != hipSuccess ||
                             hipMemsetAsync(counts_dev, 0, (size_t)ncounts * 8, ctx->stream) != hipSuccess))
            rc = GF2_E_HIP;
        for (int c = 0; c < 2 && rc == GF2_OK; ++c) {
            const int kw = kws[c];
            const size_t ent = (size_t)(es[c] > 0 ? es[c] : 1);
            rc = gf2_dev_alloc(ctx, ent * 8 * kw, &dev[c][0]);
            if (rc == GF2_OK) rc = gf2_dev_alloc(ctx, ent, &dev[c][1]);
            if (rc == GF2_OK && es[c]) rc = gf2_h2d(ctx, dev[c][0], ks[c], (size_t)es[c] * 8 * kw);
            if (rc == GF2_OK && es[c]) rc = gf2_h2d(ctx, dev[c][1], fs[c], (size_t)es[c]);
            if (rc == GF2_OK) rc = tabs[c].make(pow2_at_least((u64)es[c] * 2 + 2), kw);
            if (rc == GF2_OK && es[c]) {
                hipLaunchKernelGGL(table_insert_kernel, dim3((unsigned)gf2_cdiv(es[c], 256)), dim3(256), 0, ctx->stream, tabs[c].tab,
                                   (const u64*)dev[c][0], kw, es[c], flags_dev);
                if (hipGetLastError() != hipSuccess) rc = GF2_E_HIP;
            }
            a->tab[c] = tabs[c].tab;
            a->flips[c] = (const unsigned char*)dev[c][1];
        }
        int flags_host[2] = {0, 0};
        if (rc == GF2_OK && (hipMemcpyAsync(flags_host, flags_dev, 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                             hipStreamSynchronize(ctx->stream) != hipSuccess))
            rc = GF2_E_HIP;
        if (rc == GF2_OK && (flags_host[0] || flags_host[1])) {
            gf2_set_error(flags_host[0] ? "%s: a syndrome key occurs twice in a table" : "%s: the hash table gave up", who);
            rc = flags_host[0] ? GF2_E_ARG : GF2_E_HIP;
        }
        return rc;
    }
};

// The faults of Monte-Carlo sample `ks` XOR-ed into out[]: the sampler run over the circuit's locations segment by segment
// (cdf_lds: the two staged inverse-CDF tables), every fault's effect gathered from eff (LDS or global).  mine: this lane's 512-bit
// "taken" map for Floyd's rule, only touched by a segment with at least two faults.
template <int LDR>
__device__ __forceinline__ void circuit_gather(const SegTables& th, const u64* cdf_lds, const u64* eff, unsigned int* mine, u64 ks,
                                               u64 (&out)[LDR]) {
    for (int s = 0; s < th.nseg; ++s) {
        const bool last = s == th.nseg - 1;
        const int nb = last ? th.nb_last : GF2_SEG_BITS;
        const u64 d = segment_draw(ks, (u64)s);
        const int K = error_count(d, nb, cdf_lds + (last ? GF2_SEG_CDF : 0));
        if (K > 1)
            for (int w = 0; w < (nb + 31) >> 5; ++w) mine[w] = 0;
        for (int k = 0; k < K; ++k) {
            unsigned int t, kind;
            error_draw(d, k, K, nb, th.t_1, th.t_2, &t, &kind);
            unsigned int pos = t;
            if (K > 1) {                                                       // Floyd's rule: a candidate already taken -> j
                if ((mine[t >> 5] >> (t & 31u)) & 1u) pos = (unsigned int)(nb - K + k);
                mine[pos >> 5] |= 1u << (pos & 31u);
            }
            const u64* e = eff + (size_t)(2 * (s * GF2_SEG_BITS + (int)pos)) * LDR;   // pos < nb: a location below L
            if (kind & 1u) {
#pragma unroll
                for (int w = 0; w < LDR; ++w) out[w] ^= e[w];
            }
            if (kind & 2u) {
#pragma unroll
                for (int w = 0; w < LDR; ++w) out[w] ^= e[LDR + w];
            }
        }
    }
}
