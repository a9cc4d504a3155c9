// What gf2_host.cpp (the host statement of the repeat-until-success sampler with waiting faults) and gf2_retry_wait.hip (its device
// side) share: the argument rules of the regions' wait rows and what follows from them (include/gf2hip.h "repeat-until-success with
// waiting faults").  Plain C++, no HIP; gf2_retry_wait_plan is defined in gf2_host.cpp.
#pragma once

#include <stdint.h>

#include <vector>

#include "gf2_retry_plan.h"

// The segment slot of region 0's wait key: region g draws its wait key from slot GF2_RETRY_WAIT_SLOT_BASE + g of the sample's key,
// its own key from GF2_RETRY_SLOT_BASE + g with g < 2^20.
#define GF2_RETRY_WAIT_SLOT_BASE 8589934592ull
static_assert(GF2_RETRY_WAIT_SLOT_BASE > GF2_RETRY_SLOT_BASE + 1048576, "the wait slots lie above the regions' slots, and so above every other stream's");

#define GF2_RETRY_WAIT_MAX_ROWS 512             // wait rows of one region: one sampler segment

struct RetryWaitPlan {
    std::vector<int64_t> first;                // per region of every type (RetryPlan's numbering): its first row in wait_eff
    std::vector<int32_t> count;                // per region: its wait rows W (0: none)
    std::vector<int32_t> size;                 // per region: where W stands in `sizes` (-1 for W = 0)
    std::vector<int32_t> sizes;                // the distinct non-zero W of all regions, ascending (<= GF2_RETRY_MAX_SIZES)
    int64_t rows;                              // wait rows of all types: wait_eff holds 4 words for each
    int64_t locations;                         // wait rows per attempt, summed over the retried regions of the whole sequence
};

// Checks a sequence and its regions as gf2_retry_plan does, then the wait rows: wait_count holds W per region of every type, wait_eff
// (rows, 2, 2) the (local, tail) words of an X and of a Z fault of every row, region by region.  The wait rows' bits are added to
// plan->any_local / any_tail, so gf2_stream_check_bits judges them with the block tables'.  GF2_E_ARG with a message that names `who`
// and the rule.
int gf2_retry_wait_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                        const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                        const int64_t* type_nregions, const uint64_t* wait_eff, const int64_t* wait_count, int64_t max_attempts,
                        StreamPlan* plan, RetryPlan* retry, RetryWaitPlan* wait);

// The wait rules alone, on a plan and regions already checked: what gf2_retry_wait_plan does after gf2_retry_plan, and
// gf2_retry_gate_wait_plan after gf2_retry_gate_plan.  At most max_sizes distinct non-zero wait sizes; max_sizes_name is the constant
// the message names.
int gf2_retry_wait_rules(const char* who, int64_t ntypes, const int32_t* block_type, const int32_t* block_kind, int64_t nblocks,
                         const uint64_t* wait_eff, const int64_t* wait_count, int max_sizes, const char* max_sizes_name, StreamPlan* plan,
                         const RetryPlan& retry, RetryWaitPlan* wait);

// The waiting rates of a call: GF2_E_ARG worded as gf2_retry_check_range words the gates' rates.
int gf2_retry_wait_check_rates(const char* who, double q_x, double q_y, double q_z);
