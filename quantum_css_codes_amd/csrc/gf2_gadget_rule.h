// The argument rules of the two post-selected gadgets -- the error-correction cycle and the fault-tolerant logical measurement --
// stated once for every entry point that takes them: the ten device entry points (through ec_rule_args / ft_rule_args of
// gf2_gadget_dev.h) and the host statements of gf2_host.cpp.  A layout check (the gadget's parameters against r_1, r_2 and the
// words per effect; it returns what follows from them) and an effects check (no effect may set a bit outside the layout) per gadget.
// Plain C++, no HIP.  Every failure is GF2_E_ARG with a message under the caller's `who`.
#pragma once

#include <stdint.h>

#include "gf2hip.h"

void gf2_set_error(const char* fmt, ...);

#define GADGET_RULE_FAIL(...)       \
    do {                            \
        gf2_set_error(__VA_ARGS__); \
        return GF2_E_ARG;           \
    } while (0)

// What a checked layout gives: the measurement's number of trials (set bits of measure_mask) and its first MEASURE step (both 0
// for the cycle), and the key masks -- [0]: the r_2 bits of key_x, [1]: the r_1 bits of key_z.
struct GadgetRule {
    int trials, first_measure;
    uint64_t mask[2];
};

// Both keys of a frame share a word: key_x in the low half, key_z in the high half, bits 31 and 63 left for parities.
static inline int gadget_rule_keys(const char* who, int64_t r1, int64_t r2, GadgetRule* rule) {
    if (r1 < 1 || r2 < 1 || r1 > 31 || r2 > 31)
        GADGET_RULE_FAIL("%s: needs 1 <= r_1, r_2 <= 31 (the keys share a word), got %lld and %lld", who, (long long)r1, (long long)r2);
    rule->trials = rule->first_measure = 0;
    rule->mask[0] = (1ull << r2) - 1;
    rule->mask[1] = (1ull << r1) - 1;
    return GF2_OK;
}

// The cycle: effects of ldr = 1 + rounds + F words, [final data frame] [round 1 .. rounds] [F >= 1 flag words].
static inline int ec_rule_layout(const char* who, int64_t ldr, int64_t rounds, int64_t r1, int64_t r2, GadgetRule* rule) {
    if (int rc = gadget_rule_keys(who, r1, r2, rule)) return rc;
    if (rounds < 1 || rounds > GF2_EC_MAX_ROUNDS)
        GADGET_RULE_FAIL("%s: needs 1 <= rounds <= %d, got %lld", who, GF2_EC_MAX_ROUNDS, (long long)rounds);
    if (ldr > GF2_CIRCUIT_MAX_LDR) GADGET_RULE_FAIL("%s: needs ldr <= %d words per effect, got %lld", who, GF2_CIRCUIT_MAX_LDR, (long long)ldr);
    if (ldr < rounds + 2)
        GADGET_RULE_FAIL("%s: %lld rounds need ldr = 1 + rounds + F words with F >= 1 flag words, got %lld", who, (long long)rounds,
                         (long long)ldr);
    return GF2_OK;
}

// any: the OR of all effects, word by word (ldr words; the layout checked).  The final frame may set the keys' bits and the two
// parity bits, a round's word the keys' bits, a flag word anything.
static inline int ec_rule_effects(const char* who, const uint64_t* any, int64_t rounds, const GadgetRule& rule) {
    const uint64_t keys = rule.mask[0] | rule.mask[1] << 32;
    bool beyond = (any[0] & ~(keys | 1ull << 31 | 1ull << 63)) != 0;
    for (int64_t t = 1; t <= rounds; ++t) beyond |= (any[t] & ~keys) != 0;
    if (beyond) GADGET_RULE_FAIL("%s: the effects set bits beyond the keys' r_2 / r_1 bits, the two parity bits and the flag words", who);
    return GF2_OK;
}

// The measurement: effects of min_ldr <= ldr = nsteps + F <= GF2_FT_MAX_LDR words, [step 0 .. nsteps - 1] [F >= 1 flag words]; the
// steps with a bit in measure_mask are the trials of a majority vote.  min_ldr: the fewest words the caller takes (0: no bound).
static inline int ft_rule_layout(const char* who, int64_t ldr, int64_t min_ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1, int64_t r2,
                                 GadgetRule* rule) {
    if (int rc = gadget_rule_keys(who, r1, r2, rule)) return rc;
    if (min_ldr > 0 && (ldr < min_ldr || ldr > GF2_FT_MAX_LDR))
        GADGET_RULE_FAIL("%s: needs %lld <= ldr <= %d words per effect, got %lld", who, (long long)min_ldr, GF2_FT_MAX_LDR, (long long)ldr);
    if (ldr > GF2_FT_MAX_LDR) GADGET_RULE_FAIL("%s: needs ldr <= %d words per effect, got %lld", who, GF2_FT_MAX_LDR, (long long)ldr);
    if (nsteps < 1 || ldr < nsteps + 1)
        GADGET_RULE_FAIL("%s: needs nsteps >= 1 and ldr = nsteps + F words with F >= 1 flag words, got nsteps = %lld and ldr = %lld", who,
                         (long long)nsteps, (long long)ldr);
    if (measure_mask >> nsteps) GADGET_RULE_FAIL("%s: measure_mask has bits at or above nsteps = %lld", who, (long long)nsteps);
    rule->trials = __builtin_popcountll(measure_mask);
    if (rule->trials % 2 == 0)
        GADGET_RULE_FAIL("%s: a majority vote needs an odd number of trials, measure_mask has %d", who, rule->trials);
    rule->first_measure = __builtin_ctzll(measure_mask);
    return GF2_OK;
}

// any: as for the cycle.  An EC step's word may set the keys' bits, a MEASURE step's the bits of key_x and bit 31.
static inline int ft_rule_effects(const char* who, const uint64_t* any, int64_t nsteps, uint64_t measure_mask, const GadgetRule& rule) {
    bool beyond = false;
    for (int64_t s = 0; s < nsteps; ++s)
        beyond |= (any[s] & ~((measure_mask >> s) & 1ull ? rule.mask[0] | 1ull << 31 : rule.mask[0] | rule.mask[1] << 32)) != 0;
    if (beyond)
        GADGET_RULE_FAIL("%s: the effects set bits beyond the layout (an EC step's r_2 / r_1 key bits, a MEASURE step's r_2 key bits and bit 31)",
                         who);
    return GF2_OK;
}

#undef GADGET_RULE_FAIL
