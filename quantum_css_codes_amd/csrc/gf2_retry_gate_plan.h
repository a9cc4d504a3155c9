// What gf2_host.cpp (the host statement of the repeat-until-success sampler under gate-level faults) and gf2_retry_gate.hip (its
// device side) share: the argument rules of a block sequence's regions and of the sites inside them, and what follows from them
// (include/gf2hip.h "repeat-until-success under gate-level faults").  Plain C++, no HIP; gf2_retry_gate_plan
// is defined in gf2_host.cpp.
#pragma once

#include <stdint.h>

#include <vector>

#include "gf2_retry_plan.h"

// A region's attempt draws its two classes of sites under the key ka from the slots of the direct gate sampler, GF2_GATE_MC_SLOT_ONE
// + s and GF2_GATE_MC_SLOT_CNOT + s with s < 2048; the location version draws its segments from the slots s < 2048 of the same ka.
// The two retried samplers of one seed are therefore independent streams.
static_assert(GF2_CIRCUIT_MAX_LOCATIONS / 512 <= 2048 && GF2_GATE_MC_SLOT_ONE >= 2048 && GF2_GATE_MC_SLOT_CNOT >= GF2_GATE_MC_SLOT_ONE + 2048,
              "the inner slots of the location retry and of the two gate classes are disjoint");

struct RetryGatePlan {
    std::vector<int64_t> site_first;           // per region of every type (RetryPlan's numbering): its first site in site_loc
    std::vector<int32_t> n[2];                 // per region: its one-operand sites, its CNOT sites
    std::vector<int32_t> last_size[2];         // per region and class: where the size of its last segment stands in sizes[class] (-1: no site)
    std::vector<int32_t> sizes[2];             // per class: the distinct segment sizes of all regions, ascending (<= GF2_RETRY_MAX_SIZES)
    int32_t full_size[2];                      // per class: where 512 stands in sizes[class], -1 when no region has a whole segment
    int64_t sites;                             // sites of all types
};

// Checks a sequence and its regions as gf2_retry_plan does, then the site table: site_regions holds (n_1, n_2) per region of every
// type, site_loc the type-local first locations of the sites region by region, a region's one-operand sites before its CNOTs.
// GF2_E_ARG with a message that names `who` and the rule.
int gf2_retry_gate_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                        const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                        const int64_t* type_nregions, const int32_t* site_loc, const int64_t* site_regions, int64_t max_attempts,
                        StreamPlan* plan, RetryPlan* retry, RetryGatePlan* gate);

// The second half of gf2_retry_gate_plan alone, over regions that are already checked and filled: the site rules and the segment
// sizes of the two classes; fills *gate.  gf2_mretry_gate_plan lays it over a multi-block sequence's regions.
int gf2_retry_gate_site_rules(const char* who, const int64_t* type_locations, int64_t ntypes, const int32_t* site_loc, const int64_t* site_regions,
                              const RetryPlan& checked, RetryGatePlan* gate);
