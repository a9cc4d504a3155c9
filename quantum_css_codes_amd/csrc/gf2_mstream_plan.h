// What gf2_host.cpp (the host statements of the multi-block streamed route) and gf2_mstream.hip (its device side) share: the argument
// rules of a block sequence over several data frames and what follows from it (include/gf2hip.h "multi-block streamed programs").
// Plain C++, no HIP; gf2_mstream_plan and gf2_mstream_check_bits are defined in gf2_host.cpp.
//
// The plan holds a StreamPlan, filled as gf2_stream_plan fills it (type_offset, start, step, flag, locations, nsteps, flag_rows,
// flag_words, any_local, any_tail; trials is the number of trials of ONE measurement; has_final is false), so that a region or a
// site plan of a retried variant can be laid over it as gf2_retry_plan is laid over gf2_stream_plan's.
#pragma once

#include <stdint.h>

#include <vector>

#include "gf2_stream_plan.h"

struct MStreamPlan {
    StreamPlan seq;
    std::vector<int32_t> measure;              // nblocks: the measurement (0 .. 3, in program order) of a MEASURE block, else -1
    std::vector<uint8_t> first_trial;          // nblocks: 1 for the first MEASURE block of its measurement
    int64_t nframes, measurements;
    uint64_t any_cnot[2];                      // OR of the CNOT blocks' tail words for frame a and for frame b
};

// The frame map of a transversal CNOT a -> b on the carried words (T, and the records under GF2_MSTREAM_PROPAGATED): the x half
// (key_x, bit 31) copies a -> b, the z half (key_z, bit 63) copies b -> a.  The two lines do not interfere.
static inline void gf2_mstream_cnot_map(uint64_t* word_a, uint64_t* word_b) {
    *word_b ^= *word_a & 0x00000000FFFFFFFFull;
    *word_a ^= *word_b & 0xFFFFFFFF00000000ull;
}

// Checks a sequence (every rule of gf2_mstream_create but the null context and the overlap rule) and fills *plan.  GF2_E_ARG with a
// message that names the limit, GF2_E_NOMEM when the plan does not fit the host.
int gf2_mstream_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                     const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                     int64_t nframes, MStreamPlan* plan);

// The rules of the blocks alone (kinds, frames, measurements), which the tally shares: fills measure, first_trial, measurements,
// seq.trials and seq.nsteps of *plan.
int gf2_mstream_block_rules(const char* who, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                            int64_t nframes, MStreamPlan* plan);

// The bits a plan's effects may set given r_1 and r_2: GF2_E_ARG otherwise (and for r outside [1, 31]).
int gf2_mstream_check_bits(const char* who, const MStreamPlan& plan, int64_t r1, int64_t r2);

// GF2_E_ARG unless records is GF2_MSTREAM_REFERENCE or GF2_MSTREAM_PROPAGATED.
int gf2_mstream_check_records(const char* who, int64_t records);

// The overlap rule of the device walk: no 512-location segment of the sampler may overlap more than GF2_STREAM_MAX_OVERLAP blocks.
int gf2_mstream_check_overlap(const char* who, const MStreamPlan& plan, int64_t nblocks);
