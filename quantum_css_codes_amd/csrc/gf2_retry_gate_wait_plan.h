// What gf2_host.cpp (the host statement of the repeat-until-success sampler under gate-level faults with waiting faults) and
// gf2_retry_gate_wait.hip (its device side) share: gf2_retry_gate_plan's rules, then gf2_retry_wait_plan's wait rules with this
// route's own cap on the distinct wait sizes (include/gf2hip.h "repeat-until-success with waiting faults under gate-level faults",
// DESIGN.md section 5d).  Plain C++, no HIP; gf2_retry_gate_wait_plan is defined in gf2_host.cpp.
#pragma once

#include <stdint.h>

#include <vector>

#include "gf2_retry_gate_plan.h"
#include "gf2_retry_wait_plan.h"

// GF2_RETRY_GATE_WAIT_MAX_SIZES (gf2hip.h) caps the distinct non-zero wait sizes of a sequence.  The kernel keeps one inverse-CDF
// table per distinct size in LDS beside the 2 * GF2_RETRY_MAX_SIZES tables of the two gate classes; with every table full (513
// entries) three more are what still fits (gf2_retry_gate_wait.hip asserts the worst case).  The real gadgets have one size.
static_assert(GF2_RETRY_GATE_WAIT_MAX_SIZES <= GF2_RETRY_MAX_SIZES, "RetryWaitPlan::sizes holds at most GF2_RETRY_MAX_SIZES");

// gf2_retry_gate_plan's checks, then gf2_retry_wait_rules' with at most GF2_RETRY_GATE_WAIT_MAX_SIZES distinct wait sizes.  The wait
// rows' bits are added to plan->any_local / any_tail.  GF2_E_ARG with a message that names `who` and the rule.
int gf2_retry_gate_wait_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                             const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                             const int64_t* type_nregions, const int32_t* site_loc, const int64_t* site_regions, const uint64_t* wait_eff,
                             const int64_t* wait_count, int64_t max_attempts, StreamPlan* plan, RetryPlan* retry, RetryGatePlan* gate,
                             RetryWaitPlan* wait);
