// Open-addressing hash tables of syndrome keys on the device, shared by gf2_table.hip (the table search beyond 24 checks, the
// hashed table decode) and gf2_circuit.hip (the table decode of a circuit's final frame).
#pragma once

#include "gf2_internal.h"

#define TBL_EMPTY (~0ull)

// Slot = claim word + (two-word keys) second key word + value (weight << 32 | rank in the class, as above).  The claim word is
// the key itself (one word: below 2^63) or its HIGH word (two words: below 2^63 as well), never all ones, which means "empty";
// it is taken with one atomicCAS.  Linear probing; the table is kept at most half full.  A probe that meets its own key has
// found a second error with that syndrome: the collision the reference's `if syndrome_int in table` (css_code.py:730) reports.
// Two-word keys: the owner of a slot writes the low word and then the value (all ones until then); a probe that meets its
// high word waits for the value before it compares the low words.  Owners publish before anybody of their wavefront waits
// (claim, publish and compare are three phases of a probe step, not branches of one if), so a wait is only ever for another
// wavefront, and it is bounded all the same.
#define TBL_HASH_MAX_W 12
#define TBL_HASH_MAX_N 8192
#define TBL_HASH_MAX_ENTRIES (1ull << 28)     // errors enumerated in all; the table has twice as many slots (12 or 16 bytes each... 8 + 8 [+ 8])
#define TBL_HASH_SPIN (1u << 22)

struct HashTab {
    u64* claim;                  // slots
    u64* low;                    // slots (two-word keys only)
    u64* val;                    // slots
    u64 mask;                    // slots - 1
};

__device__ __forceinline__ u64 hash_mix(u64 z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Inserts (key -> v).  Returns 0: inserted, 1: the key is there already (collision), 2: gave up (a slot's owner did not
// publish in time, or the table is full: both reported as an error by the caller).  `active`: lanes with nothing to insert
// still walk through the phases.
template <int KW>
__device__ __forceinline__ int hash_insert(const HashTab& t, u64 khi, u64 klo, u64 v, bool active) {
    const u64 claim_word = KW == 2 ? khi : klo;
    u64 slot = hash_mix(klo ^ (KW == 2 ? hash_mix(khi + 0x9E3779B97F4A7C15ull) : 0ull)) & t.mask;
    int result = active ? -1 : 0;
    for (u64 probes = 0; __ballot(result < 0) != 0; ++probes) {
        if (probes > t.mask) {                                     // (cannot happen below half load)
            if (result < 0) result = 2;
            break;
        }
        // claim
        u64 old = 0;
        if (result < 0) old = atomicCAS(&t.claim[slot], TBL_EMPTY, claim_word);
        // publish
        if (result < 0 && old == TBL_EMPTY) {
            if (KW == 2) {
                __hip_atomic_store(&t.low[slot], klo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __atomic_thread_fence(__ATOMIC_RELEASE);
            }
            __hip_atomic_store(&t.val[slot], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            result = 0;
        }
        // compare
        if (result < 0 && old == claim_word) {
            if (KW == 1)
                result = 1;
            else {
                unsigned int spins = 0;
                while (__hip_atomic_load(&t.val[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == TBL_EMPTY && spins < TBL_HASH_SPIN) {
                    __builtin_amdgcn_s_sleep(2);
                    ++spins;
                }
                __atomic_thread_fence(__ATOMIC_ACQUIRE);
                if (spins >= TBL_HASH_SPIN)
                    result = 2;
                else if (__hip_atomic_load(&t.low[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == klo)
                    result = 1;
            }
        }
        slot = (slot + 1) & t.mask;
    }
    return result;
}

// Looks `key` up (table complete, nobody writing).  Returns the slot or ~0.
template <int KW>
__device__ __forceinline__ u64 hash_find(const HashTab& t, u64 khi, u64 klo) {
    const u64 claim_word = KW == 2 ? khi : klo;
    u64 slot = hash_mix(klo ^ (KW == 2 ? hash_mix(khi + 0x9E3779B97F4A7C15ull) : 0ull)) & t.mask;
    for (u64 probes = 0; probes <= t.mask; ++probes) {
        const u64 c = t.claim[slot];
        if (c == TBL_EMPTY) return ~0ull;
        if (c == claim_word && (KW == 1 || t.low[slot] == klo)) return slot;
        slot = (slot + 1) & t.mask;
    }
    return ~0ull;
}

static __global__ void hash_fill_kernel(HashTab tab, int kw) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= tab.mask) {
        tab.claim[i] = TBL_EMPTY;
        tab.val[i] = TBL_EMPTY;
        if (kw == 2) tab.low[i] = 0;
    }
}

// Inserts entry i of `keys` (kw words each, word 0 = low) with value i.  flags[0]: a key occurs twice, flags[1]: gave up.
static __global__ __launch_bounds__(256) void table_insert_kernel(HashTab tab, const u64* __restrict__ keys, int kw, int64_t entries,
                                                           int* __restrict__ flags) {
    const int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~(int64_t)63;
    if (base >= entries) return;                                    // whole wavefronts leave together
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < entries;
    const u64 klo = live ? keys[i * kw] : 0ull, khi = live && kw == 2 ? keys[i * kw + 1] : 0ull;
    const int res = kw == 1 ? hash_insert<1>(tab, khi, klo, (u64)i, live) : hash_insert<2>(tab, khi, klo, (u64)i, live);
    if (res == 1) atomicExch(&flags[0], 1);                         // the same key twice: not a syndrome table
    if (res == 2) atomicExch(&flags[1], 1);
}

struct HashAlloc {
    gf2_ctx* ctx;
    HashTab tab;
    u64 slots;
    HashAlloc(gf2_ctx* c) : ctx(c), tab{nullptr, nullptr, nullptr, 0}, slots(0) {}
    void release() {
        if (tab.claim) (void)gf2_dev_free(ctx, tab.claim);
        if (tab.low) (void)gf2_dev_free(ctx, tab.low);
        if (tab.val) (void)gf2_dev_free(ctx, tab.val);
        tab.claim = tab.low = tab.val = nullptr;
        slots = 0;
    }
    int make(u64 want_slots, int kw) {
        release();
        GF2_TRY(gf2_dev_alloc(ctx, want_slots * 8, (void**)&tab.claim));
        GF2_TRY(gf2_dev_alloc(ctx, want_slots * 8, (void**)&tab.val));
        if (kw == 2) GF2_TRY(gf2_dev_alloc(ctx, want_slots * 8, (void**)&tab.low));
        tab.mask = want_slots - 1;
        slots = want_slots;
        hipLaunchKernelGGL(hash_fill_kernel, dim3((unsigned)((want_slots + 255) / 256)), dim3(256), 0, ctx->stream, tab, kw);
        GF2_HIP(hipGetLastError());
        return GF2_OK;
    }
    ~HashAlloc() { release(); }
};

static u64 pow2_at_least(u64 v) {
    u64 p = 1024;
    while (p < v) p <<= 1;
    return p;
}
