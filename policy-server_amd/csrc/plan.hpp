// plan.hpp — planning of one pass over a device batch (plan.cpp): slot-plan chunks of the policy
// list, the launches they take, tile geometry and LDS layout per region, the kernel arguments.
#pragma once
#include <cstdint>
#include <vector>

#include "devbatch.hpp"

namespace kw {

// Entity range [g0, g1) of string column m for requests [r0, r1).
void str_range(const Batch& B, int m, uint64_t r0, uint64_t r1, uint64_t* g0, uint64_t* g1);

// Whether a launch of `ntiles` tiles over `grid` workgroups takes the dynamic tile schedule.
bool sched_dynamic(uint64_t ntiles, uint32_t grid, bool lds_tables);
// The static rounds S a launch of `ndesc` descriptors is handed with the counters, -1: strided, no
// counter. `dyn`: what sched_dynamic chose for the launch.
int sched_static_rounds(uint64_t ndesc, uint32_t grid, bool dyn);

// The wide groups among the pass's columns (plan->wide): column ids are the output column
// (all pairs) or the rows-mode column code ((chunk << 16) | column, as rowcol holds).
void plan_wide_groups(const Env& E, const std::vector<int32_t>& list, const std::vector<uint32_t>* rows_code,
                      int origin, PassPlan* plan);

// Plan one pass of `npol` policies (all pairs), or of row_policy[r] per batch row (rows mode),
// over the rows kb's device copy holds. A KW_E_* code when the pass cannot be planned.
// timing: print the host time of its stages (the caller's KW_BULK_DEBUG; diagnostics).
int plan_pass(const kw_env* env, kw_batch* kb, const int32_t* pols, uint32_t npol, const int32_t* row_policy,
              int origin, bool timing, PassPlan* plan);

}  // namespace kw
