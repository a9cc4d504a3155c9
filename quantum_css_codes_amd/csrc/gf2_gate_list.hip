// Malignant fault sets of the two post-selected gadgets under gate-level faults (DESIGN.md section 5e "Malignant fault sets under
// gate-level faults", include/gf2hip.h "malignant fault sets under gate-level faults"): the configurations of w <= GATE_MAX_W
// faulty gates of the error-correction cycle or of a rewritten one-qubit program -- a = w - b one-operand sites with a kind in
// {X, Y, Z} each and b CNOT sites with one of the 15 two-qubit Paulis each -- whose class byte has a bit of `select`, listed as
// records instead of counted.
//
// The walk is gate_enumerate_kernel's (gf2_gate_enumerate.hip), text of its own because that kernel's may not move: lane = subset,
// runs of up to ENUM_MAX_RUN consecutive ranks per lane, grid-strided; rank = r_s + C(n_1, a) r_c, a run unranks the two parts once
// (enum_unrank_pick on four picks each) and then steps the product order; site_loc is read once per subset, through L2, and the
// eight first locations stay in VGPRs; the 3^a 15^b kind assignments in the reflected mixed-radix Gray code, the a digits of radix
// 3 below the b digits of radix 15, the kind mask of digit value v being (v + 1) ^ ((v + 1) >> 1), so that every trip flips one bit
// of one mask: one LDR-word XOR per configuration; the flag OR first and the rule skipped for a wavefront with no accepted live
// lane; every loop with a workgroup-uniform trip count; out[] and the picks never indexed at run time.  The effect table is read
// through L2 only: lists are for low weights.
//
// Emission is gadget_list_kernel's (gf2_gadget_list.hip): a lane's class byte is formed from what ec_chain / ft_walk return; hit =
// accepted and (class & select).  The ballot of the hits is wave-uniform; when it is not zero, lane 0 adds its population count to
// the call's 64-bit counter in global memory, the base it gets back is broadcast, and hit lane l takes slot base + popcount(votes
// below l).  A record is stored, with two plain stores, only if its slot is below `capacity`; the counter runs on regardless, so it
// ends as the number of listed configurations.  One global atomic per wavefront trip that lists anything, none otherwise; no LDS, no
// bins.  The kind nibbles are decoded from the scalar trip counter t only in a wavefront that emits (the walk keeps no kappa state,
// and the number c of two-operand kinds, which the counting kernel tracks, is a function of the record: it is not tracked here).
// Slots depend on the order the wavefronts arrive in: the entry point sorts the records.
#include <algorithm>
#include <new>
#include <vector>

#include "gf2_enumerate_dev.h"
#include "gf2_gadget_dev.h"

#define GATE_MAX_W GF2_GATE_ENUMERATE_MAX_WEIGHT
#define GATE_LAUNCH_CONFIGS (1ll << 28)        // configurations per launch, as gf2_gate_enumerate.hip cuts them
static_assert(GATE_MAX_W == 4, "the picks are held four and four, and their kind masks fill word 1's 16 bits");

// gf2_host.cpp: the argument rules of a rank range of sites, shared with the host statements
int gf2_gate_check_range(const char* who, int64_t locations, const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b,
                         int64_t first_rank, int64_t count);

struct GateListArgs {
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
    unsigned int select;                       // class bits that list a configuration
    u64 capacity;                              // records the buffer holds
    u64* records;                              // [capacity][GF2_FAULT_RECORD_WORDS]
    u64* found;                                // the call's counter of listed configurations
};

// The k <= 4 picks of the subset of rank r among [0, n), n >= k (the picks from k up are 0): enum_unrank on four picks.
__device__ __forceinline__ void glist_unrank(int k, u64 r, unsigned int n, unsigned int (&pos)[GATE_MAX_W]) {
    unsigned int hi = n;
    pos[3] = k > 3 ? enum_unrank_pick<4>(r, hi) : 0u;
    pos[2] = k > 2 ? enum_unrank_pick<3>(r, hi) : 0u;
    pos[1] = k > 1 ? enum_unrank_pick<2>(r, hi) : 0u;
    pos[0] = k > 0 ? enum_unrank_pick<1>(r, hi) : 0u;
}

// enum_successor on four picks.
__device__ __forceinline__ void glist_successor(int k, unsigned int (&pos)[GATE_MAX_W]) {
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
__device__ __forceinline__ void glist_product_successor(const GateListArgs& a, unsigned int (&ps)[GATE_MAX_W], unsigned int (&pc)[GATE_MAX_W]) {
    const bool wrap = a.wa == 0 || ps[0] == (unsigned int)(a.n1 - a.wa);
    unsigned int ns[GATE_MAX_W], nc[GATE_MAX_W];
#pragma unroll
    for (int k = 0; k < GATE_MAX_W; ++k) ns[k] = ps[k], nc[k] = pc[k];
    glist_successor(a.wa, ns);
    glist_successor(a.wb, nc);
#pragma unroll
    for (int k = 0; k < GATE_MAX_W; ++k) {
        ps[k] = wrap ? (k < a.wa ? (unsigned int)k : 0u) : ns[k];
        pc[k] = wrap ? nc[k] : pc[k];
    }
}

// The first locations of the picks (0 for a pick the subset does not have).  ps[k] < n1 and pc[k] < n2 for the picks it has.
__device__ __forceinline__ void glist_locations(const GateListArgs& a, const unsigned int (&ps)[GATE_MAX_W], const unsigned int (&pc)[GATE_MAX_W],
                                                unsigned int (&ls)[GATE_MAX_W], unsigned int (&lc)[GATE_MAX_W]) {
#pragma unroll
    for (int k = 0; k < GATE_MAX_W; ++k) {
        ls[k] = k < a.wa ? (unsigned int)a.site_loc[ps[k]] : 0u;
        lc[k] = k < a.wb ? (unsigned int)a.site_loc[(unsigned int)a.n1 + pc[k]] : 0u;
    }
}

__device__ __forceinline__ unsigned int glist_select(const unsigned int (&l)[GATE_MAX_W], int j) {
    const unsigned int l0 = l[0], l1 = l[1], l2 = l[2], l3 = l[3];           // (every pick read first: enum_gray_step's comment)
    unsigned int p = l0;
    p = j == 1 ? l1 : p;
    p = j == 2 ? l2 : p;
    p = j == 3 ? l3 : p;
    return p;
}

__device__ __forceinline__ unsigned int glist_kappa(unsigned int v) { return (v + 1u) ^ ((v + 1u) >> 1); }

// Trip t > 0 of the Gray code (all of it scalar): digit j moves -- among the wa digits of radix 3 or, above them, the wb digits of
// radix 15 -- by one value; the masks of the two values differ in one bit.  Returns the index of the effect whose words are XOR-ed
// in, relative to the moving pick's first location (2 * operand + component).
__device__ __forceinline__ unsigned int glist_gray_step(unsigned int t, int wa, int& j) {
    unsigned int q = t, radix = 3u;
    j = 0;
    while (j < wa && q % 3u == 0u) q /= 3u, ++j;
    if (j == wa) {
        radix = 15u;
        while (q % 15u == 0u) q /= 15u, ++j;
    }
    const unsigned int digit = q % radix, above = q / radix;
    const unsigned int now = (above & 1u) ? radix - 1u - digit : digit, was = (above & 1u) ? radix - digit : digit - 1u;
    return (unsigned int)__builtin_ctz(glist_kappa(now) ^ glist_kappa(was));
}

// The kind masks of trip t, one nibble per pick (the record's word 1, bits 0 .. 15): digit j of t in the mixed radix, reflected when
// the number formed by the digits above it is odd, its value v giving the mask (v + 1) ^ ((v + 1) >> 1).
__device__ __forceinline__ unsigned int glist_kind_masks(int wa, int wb, unsigned int t) {
    unsigned int masks = 0, q = t;
#pragma unroll
    for (int j = 0; j < GATE_MAX_W; ++j) {
        if (j < wa + wb) {
            const unsigned int radix = j < wa ? 3u : 15u;
            const unsigned int digit = q % radix;
            q /= radix;
            masks |= glist_kappa((q & 1u) ? radix - 1u - digit : digit) << (4 * j);
        }
    }
    return masks;
}

template <int LDR, int RULE>
__global__ __launch_bounds__(CIRC_THREADS) void gate_list_kernel(GateListArgs a) {
    const u64* eff = a.eff;
    const unsigned int lane = threadIdx.x & 63u;
    const u64 below = (1ull << lane) - 1ull;                                           // the lanes below this one
    const int64_t nruns = (a.count + a.run - 1) / a.run;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < nruns; base += stride) {
        const int64_t run = base + threadIdx.x;
        const int64_t first = run * a.run;                                             // of this lane, within the launch
        // a lane without a run walks rank 0: picks 0 .. a - 1 and 0 .. b - 1, all below n_1 and n_2
        const u64 rank = first < a.count ? a.first_rank + (u64)first : 0ull;
        unsigned int ps[GATE_MAX_W], pc[GATE_MAX_W], ls[GATE_MAX_W], lc[GATE_MAX_W];
        glist_unrank(a.wa, rank % a.c1, (unsigned int)a.n1, ps);
        glist_unrank(a.wb, rank / a.c1, (unsigned int)a.n2, pc);
        for (int step = 0; step < a.run; ++step) {
            const bool live = first + step < a.count;
            if (step > 0 && live) glist_product_successor(a, ps, pc);
            glist_locations(a, ps, pc, ls, lc);
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
            for (unsigned int t = 0; t < a.nkinds; ++t) {
                if (t > 0) {
                    int j;
                    const unsigned int bit = glist_gray_step(t, a.wa, j);
                    const unsigned int one = glist_select(ls, j), two = glist_select(lc, j - a.wa);
                    const unsigned int p = j < a.wa ? one : two;
                    const u64* e = eff + (size_t)(2u * p + bit) * LDR;                 // bit = 2 * operand + component
#pragma unroll
                    for (int q = 0; q < LDR; ++q) out[q] ^= e[q];
                }
                const u64 flags = RULE == RULE_EC ? ec_flag_or<LDR>(a, out) : ft_flag_or<LDR>(a, out);
                const bool acc = live && flags == 0ull;
                if (__ballot(acc) == 0ull) continue;                                   // (wave-uniform) every live lane was rejected
                unsigned int cls = 1;
                if constexpr (RULE == RULE_EC) {
                    bool flip[2], miss[2];
                    unsigned int unmatched[2] = {0, 0};
                    ec_chain<LDR>(a, out, flip, miss, unmatched);
                    cls |= (flip[0] ? 2u : 0u) | (flip[1] ? 4u : 0u) | (miss[0] ? 8u : 0u) | (miss[1] ? 16u : 0u);
                } else {
                    unsigned int wrong_trials = 0, first_wrong = 0, unmatched[2] = {0, 0};
                    ft_walk<LDR>(a, out, wrong_trials, first_wrong, unmatched);
                    cls |= (2 * wrong_trials > (unsigned int)a.trials ? 2u : 0u) | (first_wrong != 0u ? 4u : 0u) |
                           (wrong_trials != 0u && wrong_trials != (unsigned int)a.trials ? 8u : 0u) | (unmatched[0] != 0u ? 16u : 0u) |
                           (unmatched[1] != 0u ? 32u : 0u);
                }
                const bool hit = acc && (cls & a.select) != 0u;
                const u64 votes = __ballot(hit);
                if (votes == 0ull) continue;                                           // (wave-uniform) nothing to list
                u64 got = 0;
                if (lane == 0u) got = atomicAdd(a.found, (u64)__popcll(votes));
                const u64 slot0 = (u64)__builtin_amdgcn_readfirstlane((unsigned int)got) |
                                  (u64)__builtin_amdgcn_readfirstlane((unsigned int)(got >> 32)) << 32;
                const u64 slot = slot0 + (u64)__popcll(votes & below);
                if (hit && slot < a.capacity) {                                        // (records holds max(capacity, 1) records)
                    u64* record = a.records + GF2_FAULT_RECORD_WORDS * slot;
                    record[0] = a.first_rank + (u64)first + (u64)step;
                    record[1] = (u64)glist_kind_masks(a.wa, a.wb, t) | (u64)cls << 32;
                }
            }
        }
    }
}

namespace {
struct DevBlock {                                                            // device memory freed with the object
    gf2_ctx* ctx;
    void* dev = nullptr;
    explicit DevBlock(gf2_ctx* c) : ctx(c) {}
    ~DevBlock() { (void)gf2_dev_free(ctx, dev); }
};

// n records of a call sorted by (rank, kind masks): a radix sort, 16 bits a pass from the lowest, on the key
// (rank - first_rank) 2^16 + kind masks, which differs between any two records.  The key is taken digit by digit -- pass 0 the
// kind masks, pass p > 0 bits 16 (p - 1) .. of rank - first_rank < count -- so that it needs no 64-bit product.
int gate_list_sort(const char* who, uint64_t* records, size_t n, uint64_t first_rank, uint64_t count) {
    std::vector<uint64_t> other;
    std::vector<size_t> start;
    try {
        other.resize(GF2_FAULT_RECORD_WORDS * n);
        start.resize(65537);
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory sorting %zu records", who, n);
    }
    uint64_t *src = records, *dst = other.data();
    for (int pass = 0; pass == 0 || (pass <= 4 && ((count - 1) >> (16 * (pass - 1))) != 0); ++pass) {
        auto digit = [&](const uint64_t* record) {
            return pass == 0 ? record[1] & 0xFFFFull : ((record[0] - first_rank) >> (16 * (pass - 1))) & 0xFFFFull;
        };
        std::fill(start.begin(), start.end(), (size_t)0);
        for (size_t i = 0; i < n; ++i) start[digit(src + 2 * i) + 1] += 1;
        for (size_t d = 0; d < 65536; ++d) start[d + 1] += start[d];
        for (size_t i = 0; i < n; ++i) {
            const size_t at = start[digit(src + 2 * i)]++;
            dst[2 * at] = src[2 * i];
            dst[2 * at + 1] = src[2 * i + 1];
        }
        std::swap(src, dst);
    }
    if (src != records) std::copy(src, src + GF2_FAULT_RECORD_WORDS * n, records);
    return GF2_OK;
}
}  // namespace

// The launches of a checked call: tables, site table and the zeroed counter made once, the range cut into launches of at most
// GATE_LAUNCH_CONFIGS configurations, the records downloaded if they fit and sorted by (rank, kind masks) (gate_list_sort).
template <int RULE>
static int gate_list(const char* who, gf2_ctx* ctx, const gf2_circuit* circuit, GateListArgs& a, const uint64_t* keys1, const uint8_t* flips1,
                     int64_t entries1, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, const int32_t* site_loc, int64_t n1,
                     int64_t n2, int64_t w, int64_t b, int64_t first_rank, int64_t count, uint64_t select, int64_t capacity,
                     uint64_t* records_out, int64_t* found_out) {
    const uint64_t class_bits = RULE == RULE_EC ? GF2_EC_CLASS_BITS : GF2_FT_CLASS_BITS;
    if (select == 0) GF2_FAIL(GF2_E_ARG, "%s: select names no class bit", who);
    if (select & ~class_bits)
        GF2_FAIL(GF2_E_ARG, "%s: select 0x%llx has bits outside the rule's class bits 0x%llx", who, (unsigned long long)select, (unsigned long long)class_bits);
    if (capacity < 0) GF2_FAIL(GF2_E_ARG, "%s: negative capacity", who);
    if (capacity > GF2_FAULT_LIST_MAX_CAPACITY)
        GF2_FAIL(GF2_E_ARG, "%s: capacity %lld above %lld (2^28) records", who, (long long)capacity, (long long)GF2_FAULT_LIST_MAX_CAPACITY);
    if (capacity > 0 && !records_out) GF2_FAIL(GF2_E_ARG, "%s: null buffer for %lld records", who, (long long)capacity);
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    GF2_TRY(gf2_gate_check_range(who, circuit->locations, site_loc, n1, n2, w, b, first_rank, count));
    GF2_TRY(gf2_ctx_activate(ctx));
    *found_out = 0;
    if (count == 0) return GF2_OK;                                                       // (count > 0: a <= n_1 and b <= n_2)
    CircuitTables tables(ctx);
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, 1, &a));   // (its one zeroed count is the counter)
    DevBlock sites(ctx), records(ctx);
    GF2_TRY(gf2_dev_alloc(ctx, (size_t)(n1 + n2) * 4, &sites.dev));
    GF2_TRY(gf2_h2d(ctx, sites.dev, site_loc, (size_t)(n1 + n2) * 4));
    GF2_TRY(gf2_dev_alloc(ctx, (size_t)(capacity > 0 ? capacity : 1) * GF2_FAULT_RECORD_WORDS * 8, &records.dev));
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
    a.select = (unsigned int)select;
    a.capacity = (u64)capacity;
    a.records = (u64*)records.dev;
    a.found = tables.counts_dev;
    const int64_t per_launch = GATE_LAUNCH_CONFIGS / a.nkinds;                           // subsets (at least 2^28 / 15^4)
    for (int64_t done = 0; done < count; done += per_launch) {
        a.first_rank = (u64)(first_rank + done);
        a.count = count - done < per_launch ? count - done : per_launch;
        unsigned blocks;
        enum_launch_shape(a.count, &a.run, &blocks);
        GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
        gadget_for_ldr<RULE>(circuit->ldr, [&](auto ldr) {
            hipLaunchKernelGGL((gate_list_kernel<decltype(ldr)::value, RULE>), dim3(blocks), dim3(CIRC_THREADS), 0, ctx->stream, a);
        });
        GF2_TRY(gf2_prof_end(ctx));
        GF2_HIP(hipGetLastError());
    }
    uint64_t found = 0;
    GF2_TRY(gf2_d2h(ctx, &found, tables.counts_dev, 8));
    *found_out = (int64_t)found;
    if (found == 0 || found > (uint64_t)capacity) return GF2_OK;
    GF2_TRY(gf2_d2h(ctx, records_out, records.dev, (size_t)found * GF2_FAULT_RECORD_WORDS * 8));
    return gate_list_sort(who, records_out, (size_t)found, (uint64_t)first_rank, (uint64_t)count);
}

extern "C" {

int gf2_ec_gate_enumerate_list(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                               int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                               const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank, int64_t count,
                               uint64_t select, int64_t capacity, uint64_t* records_out, int64_t* found_out) {
    const char* who = "gf2_ec_gate_enumerate_list";
    if (!ctx || !circuit || !found_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GateListArgs a = {};
    GF2_TRY(ec_rule_args(who, circuit, rounds, r1, r2, &a));
    return gate_list<RULE_EC>(who, ctx, circuit, a, keys1, flips1, entries1, keys2, flips2, entries2, site_loc, n1, n2, w, b, first_rank, count,
                              select, capacity, records_out, found_out);
}

int gf2_ft_gate_enumerate_list(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1, const uint64_t* keys1,
                               const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                               const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank, int64_t count,
                               uint64_t select, int64_t capacity, uint64_t* records_out, int64_t* found_out) {
    const char* who = "gf2_ft_gate_enumerate_list";
    if (!ctx || !circuit || !found_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GateListArgs a = {};
    GF2_TRY(ft_rule_args(who, circuit, nsteps, measure_mask, r1, r2, &a));
    return gate_list<RULE_FT>(who, ctx, circuit, a, keys1, flips1, entries1, keys2, flips2, entries2, site_loc, n1, n2, w, b, first_rank, count,
                              select, capacity, records_out, found_out);
}

}  // extern "C"
