// What gf2_host.cpp (the host statement of the repeat-until-success sampler) and gf2_retry.hip (its device side) share: the argument
// rules of a block sequence's regions and what follows from them (include/gf2hip.h "repeat-until-success").
// Plain C++, no HIP; gf2_retry_plan is defined in gf2_host.cpp.
#pragma once

#include <stdint.h>

#include <vector>

#include "gf2_stream_plan.h"

// The segment slot of region 0's key: region g of a sequence draws its key from slot GF2_RETRY_SLOT_BASE + g of the sample's key.
// Every other stream of a seed uses slots below 2^14 -- the location sampler below 2048 (L <= 2^20 in segments of 512), the gate
// classes at 4096 + s and 8192 + s with s < 2048, the strata below 353 -- and a sequence has at most 2^20 regions.
#define GF2_RETRY_SLOT_BASE 4294967296ull
static_assert(GF2_RETRY_SLOT_BASE > 8192 + 2048, "the regions' slots lie above every other stream's");

struct RetryPlan {
    std::vector<int64_t> type_first;           // ntypes + 1: a type's first region among the flat arrays below
    std::vector<int32_t> first, count, retried;   // per region of every type: its locations inside the type, whether it is retried
    std::vector<int32_t> last_size;            // per region: where the size of its last segment stands in `sizes`
    std::vector<int32_t> sizes;                // the distinct segment sizes nb of all regions, ascending (<= GF2_RETRY_MAX_SIZES)
    int32_t full_size;                         // where 512 stands in `sizes`, -1 when no region has a whole segment
    int64_t regions, preparations;             // regions and retried regions of the whole sequence, over all its blocks
};

// Checks a sequence as gf2_stream_plan does and then its regions and max_attempts (every rule of gf2_retry_words_host but those of
// the sample range and the buffers); fills both plans.  GF2_E_ARG with a message that names `who` and the rule.
int gf2_retry_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                   const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                   const int64_t* type_nregions, int64_t max_attempts, StreamPlan* plan, RetryPlan* retry);

// The second half of gf2_retry_plan alone, over a sequence plan that is already checked and filled (type_offset is read): the region
// rules, the max_attempts rule and the segment sizes; fills *retry.  gf2_mretry_plan lays it over a multi-block sequence's plan.
int gf2_retry_region_rules(const char* who, const uint64_t* type_eff, const int64_t* type_locations, int64_t ntypes, const int32_t* block_type,
                           const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions, const int64_t* type_nregions,
                           int64_t max_attempts, const StreamPlan& checked, RetryPlan* retry);

// The rates and the sample range of a call: GF2_E_ARG as the streamed route words them.
int gf2_retry_check_range(const char* who, double p_x, double p_y, double p_z, int64_t first_sample, int64_t count);
