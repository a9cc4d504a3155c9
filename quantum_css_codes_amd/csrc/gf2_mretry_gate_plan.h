// What gf2_host.cpp (the host statement of the repeat-until-success sampler of multi-block programs under gate-level faults) and
// gf2_mretry_gate.hip (its device side) share: the argument rules of a multi-block sequence with regions and sites (include/gf2hip.h
// "repeat-until-success of multi-block programs under gate-level faults").  Plain C++, no HIP;
// gf2_mretry_gate_plan is defined in gf2_host.cpp.
#pragma once

#include <stdint.h>

#include "gf2_mretry_plan.h"
#include "gf2_retry_gate_plan.h"

// gf2_mretry_plan's rules, then the site rules of gf2_retry_gate_plan laid over the regions (gf2_retry_gate_site_rules), then this
// route's own rule: the one region of a CNOT block's type has no one-operand site, so its sites are the n physical CNOTs at the
// locations 0, 2, ..., 2 n - 2.  Fills the three plans.  GF2_E_ARG with a message that names `who` and the rule.
int gf2_mretry_gate_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                         const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                         int64_t nframes, const int64_t* type_regions, const int64_t* type_nregions, const int32_t* site_loc,
                         const int64_t* site_regions, int64_t max_attempts, MStreamPlan* plan, RetryPlan* retry, RetryGatePlan* gate);
