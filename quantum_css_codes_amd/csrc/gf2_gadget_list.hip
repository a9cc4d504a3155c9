// Malignant fault sets of the two post-selected gadgets (DESIGN.md "Malignant fault sets of the cycle", "Malignant fault sets of the
// measurement"): the fault configurations of weight w <= ENUM_MAX_W of the error-correction cycle or of a rewritten one-qubit
// program whose class byte -- the byte gf2_ec_tally_host / gf2_ft_tally_host give their outcome words -- has a bit of `select`,
// listed as records (include/gf2hip.h "malignant fault sets") instead of counted.
//
// The walk is gadget_enumerate_kernel's (gf2_gadget_enumerate.hip), text of its own because that kernel's may not move: lane =
// subset, runs of up to ENUM_MAX_RUN consecutive ranks per lane, one unranking per run and the colexicographic successor after it,
// the 3^w kind assignments in the reflected ternary Gray code with one LDR-word XOR per configuration, the flag OR first and the
// wave-uniform skip when no live lane is accepted, then the rule of gf2_gadget_dev.h.  The effect table is read through L2 only:
// lists are for low weights, where the walk is short either way.
//
// Emission: a lane's class byte is formed from what ec_chain / ft_walk return; hit = accepted and (class & select).  The ballot of
// the hits is wave-uniform; when it is not zero, lane 0 adds its population count to the call's 64-bit counter in global memory, the
// base it gets back is broadcast, and hit lane l takes slot base + popcount(votes below l).  A record is stored, with plain stores,
// only if its slot is below `capacity`; the counter runs on regardless, so it ends as the number of listed configurations.  One
// global atomic per wavefront that lists anything, none otherwise; no LDS, no bins.  The kinds code is decoded from the scalar trip
// counter t only in a wavefront that emits.  Slots depend on the order the wavefronts arrive in: the entry point sorts the records.
#include <algorithm>
#include <new>
#include <vector>

#include "gf2_enumerate_dev.h"
#include "gf2_gadget_dev.h"

#define GADGET_LAUNCH_CONFIGS (1ll << 28)      // configurations per launch, as gf2_gadget_enumerate.hip cuts them

struct GadgetListArgs {
    const u64* eff;
    int locations, weight;
    unsigned int pow3;                         // 3^weight
    int run;                                   // consecutive ranks per lane
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

// The kinds code of trip t of the Gray code: digit j of t, reflected when the digits above it make an odd number (enum_gray_step).
__device__ __forceinline__ unsigned int list_kinds_code(int w, unsigned int t) {
    unsigned int code = 0, place = 1, q3 = t;
#pragma unroll
    for (int j = 0; j < ENUM_MAX_W; ++j) {
        if (j < w) {
            const unsigned int digit = q3 % 3u;
            q3 /= 3u;
            code += ((q3 & 1u) ? 2u - digit : digit) * place;
            place *= 3u;
        }
    }
    return code;
}

template <int LDR, int RULE>
__global__ __launch_bounds__(CIRC_THREADS) void gadget_list_kernel(GadgetListArgs a) {
    const int w = a.weight;
    const u64* eff = a.eff;
    const unsigned int lane = threadIdx.x & 63u;
    const u64 below = (1ull << lane) - 1ull;                                           // the lanes below this one
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
                if (hit && slot < a.capacity) {
                    u64* record = a.records + GF2_FAULT_RECORD_WORDS * slot;
                    record[0] = a.first_rank + (u64)first + (u64)step;
                    record[1] = (u64)list_kinds_code(w, t) | (u64)cls << 32;
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

// n records of a call sorted by (rank, kinds code): a radix sort, 16 bits a pass from the lowest, on the key
// (rank - first_rank) * 3^w + kinds code, which is below limit = count * 3^w <= 2^63 (gf2_enum_check_range) and differs between
// any two records.  A comparison sort of the 3 x 10^6 records of a weight-3 stratum
// dominated the whole call (DESIGN.md "Malignant fault sets of the cycle", "Speed").
int list_sort(const char* who, uint64_t* records, size_t n, uint64_t first_rank, uint64_t pow3, uint64_t limit) {
    std::vector<uint64_t> other;
    std::vector<size_t> start;
    try {
        other.resize(GF2_FAULT_RECORD_WORDS * n);
        start.resize(65537);
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory sorting %zu records", who, n);
    }
    uint64_t *src = records, *dst = other.data();
    auto key = [&](const uint64_t* record) { return (record[0] - first_rank) * pow3 + (record[1] & 0xFFFFull); };
    for (int shift = 0; shift < 64 && ((limit - 1) >> shift) != 0; shift += 16) {
        std::fill(start.begin(), start.end(), (size_t)0);
        for (size_t i = 0; i < n; ++i) start[((key(src + 2 * i) >> shift) & 0xFFFFull) + 1] += 1;
        for (size_t d = 0; d < 65536; ++d) start[d + 1] += start[d];
        for (size_t i = 0; i < n; ++i) {
            const size_t at = start[(key(src + 2 * i) >> shift) & 0xFFFFull]++;
            dst[2 * at] = src[2 * i];
            dst[2 * at + 1] = src[2 * i + 1];
        }
        std::swap(src, dst);
    }
    if (src != records) std::copy(src, src + GF2_FAULT_RECORD_WORDS * n, records);
    return GF2_OK;
}
}  // namespace

// The launches of a checked call: tables and the zeroed counter made once, the range cut into launches of at most
// GADGET_LAUNCH_CONFIGS configurations, the records downloaded if they fit and sorted by (rank, kinds code) (list_sort).
template <int RULE>
static int gadget_list(const char* who, gf2_ctx* ctx, const gf2_circuit* circuit, GadgetListArgs& a, const uint64_t* keys1, const uint8_t* flips1,
                       int64_t entries1, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, int64_t w, int64_t first_rank,
                       int64_t count, uint64_t select, int64_t capacity, uint64_t* records_out, int64_t* found_out) {
    const uint64_t class_bits = RULE == RULE_EC ? GF2_EC_CLASS_BITS : GF2_FT_CLASS_BITS;
    if (select == 0) GF2_FAIL(GF2_E_ARG, "%s: select names no class bit", who);
    if (select & ~class_bits)
        GF2_FAIL(GF2_E_ARG, "%s: select 0x%llx has bits outside the rule's class bits 0x%llx", who, (unsigned long long)select, (unsigned long long)class_bits);
    if (capacity < 0) GF2_FAIL(GF2_E_ARG, "%s: negative capacity", who);
    if (capacity > GF2_FAULT_LIST_MAX_CAPACITY)
        GF2_FAIL(GF2_E_ARG, "%s: capacity %lld above %lld (2^28) records", who, (long long)capacity, (long long)GF2_FAULT_LIST_MAX_CAPACITY);
    if (capacity > 0 && !records_out) GF2_FAIL(GF2_E_ARG, "%s: null buffer for %lld records", who, (long long)capacity);
    GF2_TRY(circuit_check_tables(who, keys1, flips1, entries1, keys2, flips2, entries2));
    GF2_TRY(gf2_enum_check_range(who, circuit->locations, w, first_rank, count));
    GF2_TRY(gf2_ctx_activate(ctx));
    *found_out = 0;
    if (count == 0) return GF2_OK;
    CircuitTables tables(ctx);
    GF2_TRY(tables.make(who, keys1, flips1, entries1, keys2, flips2, entries2, 1, &a));   // (its one zeroed count is the counter)
    DevBlock records(ctx);
    GF2_TRY(gf2_dev_alloc(ctx, (size_t)(capacity > 0 ? capacity : 1) * GF2_FAULT_RECORD_WORDS * 8, &records.dev));
    a.eff = circuit->eff_dev;
    a.locations = (int)circuit->locations;
    a.weight = (int)w;
    a.pow3 = 1;
    for (int64_t k = 0; k < w; ++k) a.pow3 *= 3u;
    a.select = (unsigned int)select;
    a.capacity = (u64)capacity;
    a.records = (u64*)records.dev;
    a.found = tables.counts_dev;
    const int64_t per_launch = GADGET_LAUNCH_CONFIGS / a.pow3;                           // subsets (at least 2^28 / 3^8)
    for (int64_t done = 0; done < count; done += per_launch) {
        a.first_rank = (u64)(first_rank + done);
        a.count = count - done < per_launch ? count - done : per_launch;
        unsigned blocks;
        enum_launch_shape(a.count, &a.run, &blocks);
        GF2_TRY(gf2_prof_begin(ctx, GF2_K_SAMPLER));
        gadget_for_ldr<RULE>(circuit->ldr, [&](auto ldr) {
            hipLaunchKernelGGL((gadget_list_kernel<decltype(ldr)::value, RULE>), dim3(blocks), dim3(CIRC_THREADS), 0, ctx->stream, a);
        });
        GF2_TRY(gf2_prof_end(ctx));
        GF2_HIP(hipGetLastError());
    }
    uint64_t found = 0;
    GF2_TRY(gf2_d2h(ctx, &found, tables.counts_dev, 8));
    *found_out = (int64_t)found;
    if (found == 0 || found > (uint64_t)capacity) return GF2_OK;
    GF2_TRY(gf2_d2h(ctx, records_out, records.dev, (size_t)found * GF2_FAULT_RECORD_WORDS * 8));
    return list_sort(who, records_out, (size_t)found, (uint64_t)first_rank, a.pow3, (uint64_t)count * a.pow3);
}

extern "C" {

int gf2_ec_enumerate_list(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                          int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, int64_t w,
                          int64_t first_rank, int64_t count, uint64_t select, int64_t capacity, uint64_t* records_out, int64_t* found_out) {
    const char* who = "gf2_ec_enumerate_list";
    if (!ctx || !circuit || !found_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GadgetListArgs a = {};
    GF2_TRY(ec_rule_args(who, circuit, rounds, r1, r2, &a));
    return gadget_list<RULE_EC>(who, ctx, circuit, a, keys1, flips1, entries1, keys2, flips2, entries2, w, first_rank, count, select, capacity,
                                records_out, found_out);
}

int gf2_ft_enumerate_list(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1, const uint64_t* keys1,
                          const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                          int64_t w, int64_t first_rank, int64_t count, uint64_t select, int64_t capacity, uint64_t* records_out,
                          int64_t* found_out) {
    const char* who = "gf2_ft_enumerate_list";
    if (!ctx || !circuit || !found_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GadgetListArgs a = {};
    GF2_TRY(ft_rule_args(who, circuit, nsteps, measure_mask, r1, r2, &a));
    return gadget_list<RULE_FT>(who, ctx, circuit, a, keys1, flips1, entries1, keys2, flips2, entries2, w, first_rank, count, select, capacity,
                                records_out, found_out);
}

}  // extern "C"
