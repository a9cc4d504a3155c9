// What gf2_host.cpp (the host statement of the repeat-until-success sampler of multi-block programs) and gf2_mretry.hip (its device
// side) share: the argument rules of a multi-block sequence with regions (include/gf2hip.h "repeat-until-success of multi-block
// programs").  Plain C++, no HIP; gf2_mretry_plan is defined in gf2_host.cpp.
#pragma once

#include <stdint.h>

#include "gf2_mstream_plan.h"
#include "gf2_retry_plan.h"

// gf2_mstream_plan's rules (not the overlap rule: regions end at block boundaries), then the region rules and the max_attempts rule
// of gf2_retry_plan laid over the embedded StreamPlan, then this route's own rule: the type of a CNOT block has one region, which is
// not retried.  Fills both plans.  GF2_E_ARG with a message that names `who` and the rule.
int gf2_mretry_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                    const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                    int64_t nframes, const int64_t* type_regions, const int64_t* type_nregions, int64_t max_attempts, MStreamPlan* plan,
                    RetryPlan* retry);
