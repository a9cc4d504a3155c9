// Circuit-level fault Monte-Carlo (DESIGN.md "Circuit faults"): a Pauli-frame simulation of a gate list (H, CNOT, IDLE) whose
// every fault location fails independently -- the question the docstrings of noisy_encode_zero / noisy_encode_plus raise
// (css_code.py:203-312: "any physical errors that occur during preparation may create many correlated errors in the code block").
//
// Frame propagation through H and CNOT is linear over GF(2), so what the final frame does to a set of outcome rows (syndrome bits,
// logical parities) is the XOR, over the faults of a sample, of one precomputed vector per (location, X or Z): the effect table
// gf2_circuit_effects makes on the host (gf2_host.cpp).  The frame itself is never stored.  One kernel template, lane = sample as in
// decode_hash_kernel (gf2_table.hip): the Monte-Carlo sampler (gf2_sampler.h, unchanged) runs over the L LOCATIONS instead of the n
// qubits, segment by segment, and every fault XORs its effect into LDR register words.  Three epilogues: store the words, bin the
// two syndrome keys (gf2_mc_run's histograms), or look the keys up in the hashed syndrome tables and tally (gf2_mc_decode_hashed's
// counts).
//
// LDS per workgroup of 256 lanes: the sampler's two inverse-CDF tables (8 KiB), the effect table when it fits CIRC_EFF_LDS_BYTES
// (otherwise every fault reads its effect through L2), one 512-bit "taken" map per lane for Floyd's rule (17 dwords apart: the odd
// stride keeps the lanes of a wavefront on different banks), and the privatised bins or the five counts.  The map is only touched
// by samples with at least two faults in a segment: a segment's first fault can meet no earlier one.
//
// STRATUM (DESIGN.md "Strata"): every sample has exactly a.weight <= CIRC_STRATUM_MAX faults in ONE segment over all L locations, so
// there is no CDF table and no map (512 bits would not cover L anyway): the earlier picks stay in registers, compared with
// constant indices in a fully unrolled loop whose every trip is guarded by the uniform k < weight.
#include <new>

#include "gf2_internal.h"
#include "gf2_circuit_dev.h"

#define CIRC_BINS_LDS 4096                     // both histograms together, privatised in LDS up to this many bins
#define CIRC_STRATUM_MAX GF2_CIRCUIT_STRATUM_MAX_WEIGHT

enum { CIRC_STORE = 0, CIRC_HIST = 1, CIRC_TALLY = 2 };

struct CircuitArgs {
    const u64* eff;
    int locations;
    u64 seed;
    int64_t first_sample, count;
    SegTables th;
    int weight;                                // STRATUM only: faults per sample (th carries t_1 and t_2 only)
    // store
    u64* out;
    int64_t ldo;
    // histograms and tally: the words are [key_x: kwx] [key_z: kwz] [parity]
    int kwx, kwz;
    int mode, nbz, nbx, priv;
    u64* hist_z;
    u64* hist_x;
    HashTab tab[2];                            // [0]: parity_check_c2's table (key_x), [1]: parity_check_c1's (key_z)
    const unsigned char* flips[2];             // operator . correction of every table entry
    u64* counts;
};

// The faults of a stratified sample XOR-ed into out[]: the at most CIRC_STRATUM_MAX earlier picks in registers (constant indices after
// unrolling: nothing goes to scratch), every trip guarded by the uniform k < a.weight.
template <int LDR>
__device__ __forceinline__ void stratum_faults(const CircuitArgs& a, const u64* eff, u64 ks, u64 (&out)[LDR]) {
    const u64 d = segment_draw(ks, (u64)a.weight);
    unsigned int picks[CIRC_STRATUM_MAX];
#pragma unroll
    for (int k = 0; k < CIRC_STRATUM_MAX; ++k) {
        if (k < a.weight) {
            unsigned int t, kind;
            error_draw(d, k, a.weight, a.locations, a.th.t_1, a.th.t_2, &t, &kind);
            bool seen = false;
#pragma unroll
            for (int q = 0; q < k; ++q) seen |= picks[q] == t;
            picks[k] = seen ? (unsigned int)(a.locations - a.weight + k) : t;              // Floyd's rule; below L either way
            const u64* e = eff + (size_t)(2 * picks[k]) * LDR;
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

template <int LDR, int EPI, bool STAGED, bool STRATUM = false>
__global__ __launch_bounds__(CIRC_THREADS) void circuit_kernel(CircuitArgs a) {
    extern __shared__ u64 circ_lds[];
    u64* cdf_lds = circ_lds;                                                       // [2][GF2_SEG_CDF]  (STRATUM: neither tables nor maps)
    u64* eff_lds = circ_lds + (STRATUM ? 0 : 2 * GF2_SEG_CDF);
    unsigned int* taken = (unsigned int*)(eff_lds + (STAGED ? 2 * a.locations * LDR : 0));
    unsigned int* bins = taken + (STRATUM ? 0 : CIRC_THREADS * CIRC_TAKEN_STRIDE);  // histograms: nbz + nbx; tally: 5
    if (!STRATUM)
        for (int i = threadIdx.x; i < 2 * GF2_SEG_CDF; i += blockDim.x)
            if (a.th.nseg > 1 || i >= GF2_SEG_CDF) cdf_lds[i] = a.th.cdf[i];        // (one segment: only the last one's table is read)
    if (STAGED)
        for (int i = threadIdx.x; i < 2 * a.locations * LDR; i += blockDim.x) eff_lds[i] = a.eff[i];
    if (EPI == CIRC_HIST && a.priv)
        for (int i = threadIdx.x; i < a.nbz + a.nbx; i += blockDim.x) bins[i] = 0;
    if (EPI == CIRC_TALLY && threadIdx.x < 5) bins[threadIdx.x] = 0;
    __syncthreads();
    const u64* eff = STAGED ? eff_lds : a.eff;
    unsigned int* mine = taken + threadIdx.x * CIRC_TAKEN_STRIDE;
    unsigned int local[5] = {0, 0, 0, 0, 0};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += stride) {
        const u64 ks = sample_key(a.seed, (u64)(a.first_sample + i));
        u64 out[LDR];
#pragma unroll
        for (int w = 0; w < LDR; ++w) out[w] = 0;
        if constexpr (STRATUM) stratum_faults<LDR>(a, eff, ks, out);
        if constexpr (!STRATUM) circuit_gather<LDR>(a.th, cdf_lds, eff, mine, ks, out);
        if constexpr (EPI == CIRC_STORE) {
#pragma unroll
            for (int w = 0; w < LDR; ++w) a.out[i * a.ldo + w] = out[w];
        } else {
            // (constant indices and selects: a run-time index into out[] would put it into scratch)
            const u64 x_lo = out[0], x_hi = a.kwx == 2 ? out[1] : 0ull;
            const u64 z_lo = a.kwx == 1 ? out[1] : out[2];
            const u64 z_hi = a.kwz == 2 ? (a.kwx == 1 ? out[2] : out[LDR >= 4 ? 3 : 0]) : 0ull;
            const u64 parity = out[LDR - 1];
            if constexpr (EPI == CIRC_HIST) {
                const bool full = a.mode == GF2_HIST_FULL;
                const unsigned int bx = full ? (unsigned int)x_lo : (unsigned int)(__popcll(x_lo) + __popcll(x_hi));
                const unsigned int bz = full ? (unsigned int)z_lo : (unsigned int)(__popcll(z_lo) + __popcll(z_hi));
                if (bz < (unsigned int)a.nbz && bx < (unsigned int)a.nbx) {        // (the host has checked the table: always)
                    if (a.priv) {
                        atomicAdd(&bins[bz], 1u);
                        atomicAdd(&bins[a.nbz + bx], 1u);
                    } else {
                        atomicAdd(&a.hist_z[bz], 1ull);
                        atomicAdd(&a.hist_x[bx], 1ull);
                    }
                }
            } else {
                bool flip[2], miss[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const u64 lo = c ? z_lo : x_lo, hi = c ? z_hi : x_hi;
                    const int kw = c ? a.kwz : a.kwx;
                    const u64 slot = kw == 1 ? hash_find<1>(a.tab[c], 0ull, lo) : hash_find<2>(a.tab[c], hi, lo);
                    miss[c] = slot == ~0ull;
                    flip[c] = (parity >> c) & 1ull;
                    if (!miss[c]) flip[c] = flip[c] != (bool)(a.flips[c][a.tab[c].val[slot]] & 1);   // css_code.py:655-657: no match, no correction
                }
                local[0] += flip[0];
                local[1] += flip[1];
                local[2] += flip[0] | flip[1];
                local[3] += miss[0];
                local[4] += miss[1];
            }
        }
    }
    if (EPI == CIRC_HIST && a.priv) {
        __syncthreads();
        for (int i = threadIdx.x; i < a.nbz; i += blockDim.x)
            if (bins[i]) atomicAdd(&a.hist_z[i], (u64)bins[i]);
        for (int i = threadIdx.x; i < a.nbx; i += blockDim.x)
            if (bins[a.nbz + i]) atomicAdd(&a.hist_x[i], (u64)bins[a.nbz + i]);
    }
    if (EPI == CIRC_TALLY) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (local[k]) atomicAdd(&bins[k], local[k]);
        __syncthreads();
        if (threadIdx.x < 5 && bins[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (u64)bins[threadIdx.x]);
    }
}

template <int LDR, int EPI>
static void circuit_launch_ldr(gf2_ctx* ctx, const CircuitArgs& a, bool staged, bool stratum, unsigned blocks, size_t lds) {
    if constexpr (EPI == CIRC_TALLY && LDR >= 3 && LDR <= 5) {
        if (stratum) {
            if (staged)
                hipLaunchKernelGGL((circuit_kernel<LDR, EPI, true, true>), dim3(blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
            else
                hipLaunchKernelGGL((circuit_kernel<LDR, EPI, false, true>), dim3(blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
            return;
        }
    }
    if (staged)
        hipLaunchKernelGGL((circuit_kernel<LDR, EPI, true>), dim3(blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    else
        hipLaunchKernelGGL((circuit_kernel<LDR, EPI, false>), dim3(blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
}

// bins: LDS dwords behind the taken maps.  The histogram and tally epilogues exist for the 3 to 5 words of the Monte-Carlo layout.
// (stratum: the tally epilogue only)
template <int EPI>
static int circuit_launch(gf2_ctx* ctx, const gf2_circuit* circ, CircuitArgs& a, int bins, bool stratum = false) {
    const size_t eff_bytes = (size_t)2 * circ->locations * circ->ldr * 8;
    const bool staged = eff_bytes <= CIRC_EFF_LDS_BYTES;
    const size_t lds = (stratum ? 0 : (size_t)2 * GF2_SEG_CDF * 8 + (size_t)CIRC_THREADS * CIRC_TAKEN_STRIDE * 4) + (staged ? eff_bytes : 0) +
                       (size_t)bins * 4;
    a.eff = circ->eff_dev;
    a.locations = (int)circ->locations;
    int64_t blocks = gf2_cdiv(a.count, CIRC_THREADS * 16);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
    switch (circ->ldr) {
        case 3: circuit_launch_ldr<3, EPI>(ctx, a, staged, stratum, (unsigned)blocks, lds); break;
        case 4: circuit_launch_ldr<4, EPI>(ctx, a, staged, stratum, (unsigned)blocks, lds); break;
        case 5: circuit_launch_ldr<5, EPI>(ctx, a, staged, stratum, (unsigned)blocks, lds); break;
        default:
            if (EPI == CIRC_STORE) switch (circ->ldr) {
                case 1: circuit_launch_ldr<1, CIRC_STORE>(ctx, a, staged, false, (unsigned)blocks, lds); break;
                case 2: circuit_launch_ldr<2, CIRC_STORE>(ctx, a, staged, false, (unsigned)blocks, lds); break;
                case 6: circuit_launch_ldr<6, CIRC_STORE>(ctx, a, staged, false, (unsigned)blocks, lds); break;
                case 7: circuit_launch_ldr<7, CIRC_STORE>(ctx, a, staged, false, (unsigned)blocks, lds); break;
                case 8: circuit_launch_ldr<8, CIRC_STORE>(ctx, a, staged, false, (unsigned)blocks, lds); break;
            }
    }
    GF2_TRY(gf2_prof_end(ctx));
    GF2_HIP(hipGetLastError());
    return GF2_OK;
}

int gf2_circuit_create_upto(const char* who, gf2_ctx* ctx, const uint64_t* eff, int64_t locations, int64_t ldr, int64_t max_ldr,
                            gf2_circuit** circuit_out) {
    if (!ctx || !eff || !circuit_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    *circuit_out = nullptr;
    if (locations < 1 || locations > GF2_CIRCUIT_MAX_LOCATIONS)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= locations <= %d (2^20), got %lld", who, GF2_CIRCUIT_MAX_LOCATIONS, (long long)locations);
    if (ldr < 1 || ldr > max_ldr)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= ldr <= %d words per effect, got %lld", who, (int)max_ldr, (long long)ldr);
    GF2_TRY(gf2_ctx_activate(ctx));
    gf2_circuit* circ = new (std::nothrow) gf2_circuit();
    if (!circ) GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    circ->locations = locations;
    circ->ldr = ldr;
    circ->eff_dev = nullptr;
    for (int w = 0; w < GF2_FT_MAX_LDR; ++w) circ->any[w] = 0;
    for (int64_t i = 0; i < 2 * locations; ++i)
        for (int64_t w = 0; w < ldr; ++w) circ->any[w] |= eff[i * ldr + w];
    const size_t bytes = (size_t)2 * locations * ldr * 8;
    int rc = gf2_dev_alloc(ctx, bytes, (void**)&circ->eff_dev);
    if (rc == GF2_OK) rc = gf2_h2d(ctx, circ->eff_dev, eff, bytes);
    if (rc != GF2_OK) {
        if (circ->eff_dev) (void)gf2_dev_free(ctx, circ->eff_dev);
        delete circ;
        return rc;
    }
    *circuit_out = circ;
    return GF2_OK;
}

extern "C" {

int gf2_circuit_create(gf2_ctx* ctx, const uint64_t* eff, int64_t locations, int64_t ldr, gf2_circuit** circuit_out) {
    return gf2_circuit_create_upto("gf2_circuit_create", ctx, eff, locations, ldr, GF2_CIRCUIT_MAX_LDR, circuit_out);
}

int gf2_circuit_destroy(gf2_ctx* ctx, gf2_circuit* circuit) {
    if (!ctx) GF2_FAIL(GF2_E_ARG, "gf2_circuit_destroy: null context");
    if (!circuit) return GF2_OK;
    const int rc = gf2_dev_free(ctx, circuit->eff_dev);
    delete circuit;
    return rc;
}

int gf2_circuit_outcomes_dev(gf2_ctx* ctx, const gf2_circuit* circuit, uint64_t seed, int64_t first_sample, int64_t count,
                             double p_x, double p_y, double p_z, uint64_t* out_dev, int64_t ldo) {
    if (!ctx || !circuit) GF2_FAIL(GF2_E_ARG, "gf2_circuit_outcomes_dev: null argument");
    if (circuit->ldr > GF2_CIRCUIT_MAX_LDR)                               // (a gf2_ft_circuit_create one: gf2_ft_outcomes_dev stores it)
        GF2_FAIL(GF2_E_ARG, "gf2_circuit_outcomes_dev: needs ldr <= %d words per sample, got %lld", GF2_CIRCUIT_MAX_LDR, (long long)circuit->ldr);
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "gf2_circuit_outcomes_dev: negative range");
    if (ldo < circuit->ldr) GF2_FAIL(GF2_E_ARG, "gf2_circuit_outcomes_dev: ldo must be at least the circuit's %lld words", (long long)circuit->ldr);
    GF2_TRY(check_probabilities(p_x, p_y, p_z));
    if (count == 0) return GF2_OK;
    if (!out_dev) GF2_FAIL(GF2_E_ARG, "gf2_circuit_outcomes_dev: null buffer");
    GF2_TRY(gf2_ctx_activate(ctx));
    CircuitArgs a = {};
    GF2_TRY(gf2_seg_tables(ctx, p_x, p_y, p_z, circuit->locations, &a.th));
    a.seed = seed;
    a.first_sample = first_sample;
    a.count = count;
    a.out = (u64*)out_dev;
    a.ldo = ldo;
    return circuit_launch<CIRC_STORE>(ctx, circuit, a, 0);
}

int gf2_mc_circuit_run(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t r1, int64_t r2, uint64_t seed, int64_t first_sample,
                       int64_t count, double p_x, double p_y, double p_z, int mode, uint64_t* hist_z, int64_t nbins_z,
                       uint64_t* hist_x, int64_t nbins_x) {
    if (!ctx || !circuit || !hist_z || !hist_x) GF2_FAIL(GF2_E_ARG, "gf2_mc_circuit_run: null argument");
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "gf2_mc_circuit_run: negative range");
    if (mode != GF2_HIST_FULL && mode != GF2_HIST_WEIGHT) GF2_FAIL(GF2_E_ARG, "gf2_mc_circuit_run: unknown mode %d", mode);
    CircuitArgs a = {};
    GF2_TRY(circuit_layout("gf2_mc_circuit_run", circuit, r1, r2, &a));
    if (mode == GF2_HIST_FULL && (r1 > 24 || r2 > 24)) GF2_FAIL(GF2_E_ARG, "gf2_mc_circuit_run: full histograms need r <= 24");
    const int64_t want_z = mode == GF2_HIST_FULL ? (1ll << r1) : r1 + 1, want_x = mode == GF2_HIST_FULL ? (1ll << r2) : r2 + 1;
    if (nbins_z != want_z || nbins_x != want_x)
        GF2_FAIL(GF2_E_ARG, "gf2_mc_circuit_run: expected %lld and %lld bins", (long long)want_z, (long long)want_x);
    GF2_TRY(check_probabilities(p_x, p_y, p_z));
    GF2_TRY(gf2_ctx_activate(ctx));
    const size_t hzb = (size_t)nbins_z * 8, hxb = (size_t)nbins_x * 8;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    GF2_TRY(gf2_ws_reserve(ctx, 0, al(hzb) + al(hxb)));
    uint64_t* dz = (uint64_t*)ctx->ws[0];
    uint64_t* dx = (uint64_t*)((char*)ctx->ws[0] + al(hzb));
    GF2_TRY(gf2_dev_zero(ctx, dz, hzb));
    GF2_TRY(gf2_dev_zero(ctx, dx, hxb));
    if (count > 0) {
        GF2_TRY(gf2_seg_tables(ctx, p_x, p_y, p_z, circuit->locations, &a.th));
        a.seed = seed;
        a.first_sample = first_sample;
        a.count = count;
        a.mode = mode;
        a.nbz = (int)nbins_z;
        a.nbx = (int)nbins_x;
        a.priv = nbins_z + nbins_x <= CIRC_BINS_LDS;
        a.hist_z = (u64*)dz;
        a.hist_x = (u64*)dx;
        GF2_TRY(circuit_launch<CIRC_HIST>(ctx, circuit, a, a.priv ? (int)(nbins_z + nbins_x) : 0));
    }
    GF2_TRY(gf2_d2h(ctx, hist_z, dz, hzb));
    GF2_TRY(gf2_d2h(ctx, hist_x, dx, hxb));
    return GF2_OK;
}

int gf2_mc_circuit_decode(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                          int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                          uint64_t seed, int64_t first_sample, int64_t count, double p_x, double p_y, double p_z,
                          uint64_t* counts_out) {
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "gf2_mc_circuit_decode: null argument");
    CircuitArgs a = {};
    GF2_TRY(circuit_layout("gf2_mc_circuit_decode", circuit, r1, r2, &a));
    GF2_TRY(circuit_check_tables("gf2_mc_circuit_decode", keys1, flips1, entries1, keys2, flips2, entries2));
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "gf2_mc_circuit_decode: negative range");
    GF2_TRY(check_probabilities(p_x, p_y, p_z));
    GF2_TRY(gf2_ctx_activate(ctx));
    for (int k = 0; k < 5; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    GF2_TRY(gf2_seg_tables(ctx, p_x, p_y, p_z, circuit->locations, &a.th));
    a.seed = seed;
    a.first_sample = first_sample;
    a.count = count;
    CircuitTables tables(ctx);
    GF2_TRY(tables.make("gf2_mc_circuit_decode", keys1, flips1, entries1, keys2, flips2, entries2, 5, &a));
    a.counts = tables.counts_dev;
    GF2_TRY(circuit_launch<CIRC_TALLY>(ctx, circuit, a, 5));
    return gf2_d2h(ctx, counts_out, tables.counts_dev, 40);
}

int gf2_mc_circuit_decode_strata(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                                 int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                                 uint64_t seed, int64_t first_sample, int64_t nstrata, const int32_t* weights, const int64_t* counts,
                                 double k_x, double k_y, double k_z, uint64_t* counts_out) {
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "gf2_mc_circuit_decode_strata: null argument");
    CircuitArgs a = {};
    GF2_TRY(circuit_layout("gf2_mc_circuit_decode_strata", circuit, r1, r2, &a));
    GF2_TRY(circuit_check_tables("gf2_mc_circuit_decode_strata", keys1, flips1, entries1, keys2, flips2, entries2));
    if (nstrata < 0 || nstrata > GF2_STRATA_MAX || (nstrata && (!weights || !counts)))
        GF2_FAIL(GF2_E_ARG, "gf2_mc_circuit_decode_strata: needs 0 <= nstrata <= %d and their weights and counts", GF2_STRATA_MAX);
    if (first_sample < 0) GF2_FAIL(GF2_E_ARG, "gf2_mc_circuit_decode_strata: negative range");
    int64_t total = 0;
    for (int64_t s = 0; s < nstrata; ++s) {
        if (weights[s] < 0 || weights[s] > CIRC_STRATUM_MAX || weights[s] > circuit->locations)
            GF2_FAIL(GF2_E_ARG, "gf2_mc_circuit_decode_strata: stratum %lld has weight %d outside [0, min(L = %lld, %d)]", (long long)s,
                     (int)weights[s], (long long)circuit->locations, CIRC_STRATUM_MAX);
        if (counts[s] < 0) GF2_FAIL(GF2_E_ARG, "gf2_mc_circuit_decode_strata: stratum %lld has a negative sample count", (long long)s);
        total += counts[s] > 0;
    }
    GF2_TRY(stratum_thresholds("gf2_mc_circuit_decode_strata", k_x, k_y, k_z, &a.th.t_1, &a.th.t_2));
    GF2_TRY(gf2_ctx_activate(ctx));
    for (int64_t k = 0; k < 5 * nstrata; ++k) counts_out[k] = 0;
    if (total == 0) return GF2_OK;
    a.seed = seed;
    a.first_sample = first_sample;
    CircuitTables tables(ctx);
    GF2_TRY(tables.make("gf2_mc_circuit_decode_strata", keys1, flips1, entries1, keys2, flips2, entries2, 5 * nstrata, &a));
    for (int64_t s = 0; s < nstrata; ++s) {
        if (counts[s] == 0) continue;
        a.weight = (int)weights[s];
        a.count = counts[s];
        a.counts = tables.counts_dev + 5 * s;
        GF2_TRY(circuit_launch<CIRC_TALLY>(ctx, circuit, a, 5, true));
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, (size_t)nstrata * 40);
}

}  // extern "C"
