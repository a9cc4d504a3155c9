// What gf2_host.cpp (the host statements of the streamed route) and gf2_stream.hip (its device side) share: the argument rules of a
// block sequence and what follows from it -- where every block's locations, step word and flag rows lie (include/gf2hip.h "streamed
// gadgets").  Plain C++, no HIP; gf2_stream_plan is defined in gf2_host.cpp.
#pragma once

#include <stdint.h>

#include <vector>

struct StreamPlan {
    std::vector<int64_t> type_offset;          // ntypes: first location of a type's table in type_eff
    std::vector<int32_t> start;                // nblocks + 1: first location of every block, then L
    std::vector<int32_t> step;                 // nblocks: the block's step (its word in the stream layout), -1 for a NONE block
    std::vector<int32_t> flag;                 // nblocks: the block's first flag row
    int64_t locations, nsteps, flag_rows, flag_words, trials;
    bool has_final;
    uint64_t any_local[4], any_tail;           // OR of the local words of the blocks of every kind, and of all tail words
};

// The step words' r-free masks: what of the data frame T a step of a kind reads (an EC step the two keys, a MEASURE step key_x and
// the z_operator parity, the FINAL step everything).  T only has bits of the layout, so no r enters.
static inline uint64_t gf2_stream_frame_mask(int kind) {
    return kind == GF2_STREAM_EC ? ~(1ull << 31 | 1ull << 63) : kind == GF2_STREAM_MEASURE ? 0xFFFFFFFFull : kind == GF2_STREAM_FINAL ? ~0ull : 0ull;
}

// Checks a sequence (every rule of gf2_stream_create but the null context) and fills *plan.  GF2_E_ARG with a message that names the
// limit, GF2_E_NOMEM when the plan does not fit the host.
int gf2_stream_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                    const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, StreamPlan* plan);

// The bits a plan's effects may set given r_1 and r_2: GF2_E_ARG otherwise (and for r outside [1, 31]).
int gf2_stream_check_bits(const char* who, const StreamPlan& plan, int64_t r1, int64_t r2);
