// Exact strata (DESIGN.md "Exact strata"): every fault configuration of weight w <= ENUM_MAX_W of a circuit -- a subset S of the L
// locations with a kind in {X, Y, Z} per pick -- decoded and tallied by circuit_kernel's rule (gf2_circuit.hip), counted per kind
// composition (n_x, n_y).  Nothing is sampled: the subsets are the ranks [first_rank, first_rank + count) of the combinatorial
// number system, rank(S) = sum_k C(s_k, k + 1).
//
// Lane = subset.  A lane takes a run of a.run consecutive ranks (runs grid-strided): it unranks the first (a binary search per
// pick over exact binomials: 64-bit multiplies and constant divisors, paid once per run) and steps to the colexicographic
// successor for the others.  The 3^w kind assignments of a subset are walked in the reflected ternary Gray code over the digit
// order X, Y, Z: trip t changes digit j = (number of times 3 divides t) by one step, X <-> Y XORs that pick's Z effect, Y <-> Z
// its X effect -- one LDR-word XOR per configuration, no random numbers.  t, j, the step and with them the composition are the
// same in every lane of the grid (scalar registers), the picks stay in eight VGPRs chosen by selects on the scalar j, and every
// loop has a workgroup-uniform trip count: lanes without a subset walk along with `live` off.
//
// Tallies: the composition is wave-uniform, so a field's count over the wavefront is the population count of a ballot, added by
// one lane to the workgroup's LDS bins [n_x][n_y][5] (at most 405 dwords; a launch covers at most ENUM_LAUNCH_CONFIGS < 2^32
// configurations) only when it is non-zero; the bins go to global memory once per workgroup.
#include "gf2_enumerate_dev.h"

struct EnumArgs {
    const u64* eff;
    int locations, weight;
    unsigned int pow3;                         // 3^weight
    int run;                                   // consecutive ranks per lane
    u64 first_rank;
    int64_t count;                             // subsets of this launch
    int kwx, kwz;
    HashTab tab[2];
    const unsigned char* flips[2];
    u64* counts;                               // [(weight + 1)][(weight + 1)][5]
};

template <int LDR, bool STAGED>
__global__ __launch_bounds__(CIRC_THREADS) void enumerate_kernel(EnumArgs a) {
    extern __shared__ u64 enum_lds[];
    u64* eff_lds = enum_lds;
    unsigned int* bins = (unsigned int*)(eff_lds + (STAGED ? 2 * a.locations * LDR : 0));
    const int w = a.weight, side = w + 1, nbins = side * side * 5;
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
        unsigned int pos[ENUM_MAX_W];
        // a lane without a run unranks rank 0: picks 0 .. w - 1, all below L
        enum_unrank(w, first < a.count ? a.first_rank + (u64)first : 0ull, (unsigned int)a.locations, pos);
        for (int step = 0; step < a.run; ++step) {
            const bool live = first + step < a.count;
            if (step > 0 && live) enum_successor(w, pos);
            u64 out[LDR];
            enum_all_x<LDR>(w, eff, pos, out);                                         // all X
            int n_x = w, n_y = 0;
            for (unsigned int t = 0; t < a.pow3; ++t) {
                if (t > 0) {
                    bool xy;
                    const unsigned int p = enum_gray_step(t, pos, xy, n_x, n_y);
                    const u64* e = eff + (size_t)(2 * p + (xy ? 1u : 0u)) * LDR;
#pragma unroll
                    for (int q = 0; q < LDR; ++q) out[q] ^= e[q];
                }
                const u64 x_lo = out[0], x_hi = a.kwx == 2 ? out[1] : 0ull;
                const u64 z_lo = a.kwx == 1 ? out[1] : out[2];
                const u64 z_hi = a.kwz == 2 ? (a.kwx == 1 ? out[2] : out[LDR >= 4 ? 3 : 0]) : 0ull;
                const u64 parity = out[LDR - 1];
                bool flip[2], miss[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const u64 lo = c ? z_lo : x_lo, hi = c ? z_hi : x_hi;
                    const int kw = c ? a.kwz : a.kwx;
                    const u64 slot = kw == 1 ? hash_find<1>(a.tab[c], 0ull, lo) : hash_find<2>(a.tab[c], hi, lo);
                    miss[c] = slot == ~0ull;
                    flip[c] = (parity >> c) & 1ull;
                    if (!miss[c]) flip[c] = flip[c] != (bool)(a.flips[c][a.tab[c].val[slot]] & 1);
                }
                unsigned int* bin = bins + (n_x * side + n_y) * 5;
                const u64 votes[5] = {__ballot(live && flip[0]), __ballot(live && flip[1]), __ballot(live && (flip[0] || flip[1])),
                                      __ballot(live && miss[0]), __ballot(live && miss[1])};
#pragma unroll
                for (int f = 0; f < 5; ++f)
                    if (votes[f] != 0ull && first_lane) atomicAdd(&bin[f], (unsigned int)__popcll(votes[f]));
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nbins; i += blockDim.x)
        if (bins[i]) atomicAdd(&a.counts[i], (u64)bins[i]);
}

template <int LDR>
static void enumerate_launch_ldr(gf2_ctx* ctx, const EnumArgs& a, bool staged, unsigned blocks, size_t lds) {
    if (staged)
        hipLaunchKernelGGL((enumerate_kernel<LDR, true>), dim3(blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
    else
        hipLaunchKernelGGL((enumerate_kernel<LDR, false>), dim3(blocks), dim3(CIRC_THREADS), lds, ctx->stream, a);
}

extern "C" int gf2_circuit_enumerate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                                     int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                                     int64_t w, int64_t first_rank, int64_t count, uint64_t* counts_out) {
    const char* who = "gf2_circuit_enumerate";
    if (!ctx || !circuit || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    EnumArgs a = {};
    GF2_TRY(circuit_layout(who, circuit, r1, r2, &a));
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    GF2_TRY(gf2_enum_check_range(who, circuit->locations, w, first_rank, count));
    GF2_TRY(gf2_ctx_activate(ctx));
    const int64_t ncounts = (w + 1) * (w + 1) * 5;
    for (int64_t k = 0; k < ncounts; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    CircuitTables tables(ctx);
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, ncounts, &a));
    a.eff = circuit->eff_dev;
    a.locations = (int)circuit->locations;
    a.weight = (int)w;
    a.pow3 = 1;
    for (int64_t k = 0; k < w; ++k) a.pow3 *= 3u;
    a.counts = tables.counts_dev;
    size_t lds;
    const bool staged = circuit_staged(circuit, true, (size_t)ncounts * 4, &lds);
    const int64_t per_launch = ENUM_LAUNCH_CONFIGS / a.pow3;                             // subsets (at least 2^30 / 3^8)
    for (int64_t done = 0; done < count; done += per_launch) {
        a.first_rank = (u64)(first_rank + done);
        a.count = count - done < per_launch ? count - done : per_launch;
        unsigned blocks;
        enum_launch_shape(a.count, &a.run, &blocks);
        GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
        switch (circuit->ldr) {                                                          // (circuit_layout: 3, 4 or 5)
            case 3: enumerate_launch_ldr<3>(ctx, a, staged, blocks, lds); break;
            case 4: enumerate_launch_ldr<4>(ctx, a, staged, blocks, lds); break;
            case 5: enumerate_launch_ldr<5>(ctx, a, staged, blocks, lds); break;
        }
        GF2_TRY(gf2_prof_end(ctx));
        GF2_HIP(hipGetLastError());
    }
    return gf2_d2h(ctx, counts_out, tables.counts_dev, (size_t)ncounts * 8);
}
