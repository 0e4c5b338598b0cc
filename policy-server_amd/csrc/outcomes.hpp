// outcomes.hpp — the pure arithmetic of the grouped outcome count (include/kwgpu.h kw_batch_outcomes):
// the 9-valued outcome of a verdict word, which is everything Metrics::record (metrics.cpp) reads
// from it; the reference host reducer over words [rows][npol] and a group id per row; and the
// geometry of the device count (reports.hip outcomes_kernel): the counting sort of the rows by
// group, the unit table and the cut of the groups into ranges whose table fits a byte budget.
// No HIP, no batch, no settings (tests/outcomes_check.cpp runs it on the host).
//
// What the table replaces: the label set of a (row, policy) pair of
// kubewarden_policy_evaluations_total (src/metrics.rs:49-140) is (attributes of the row) x (policy)
// x (outcome of the word), and a row's attributes do not depend on the policy. With the rows'
// attribute sets numbered once (kw_batch_attribute_groups), out[group][outcome][column] holds every
// series' count of a pass.
#pragma once
#include <cstddef>
#include <cstdint>

#include "packed.hpp"
#include "slots.hpp"

namespace kw {

// The outcome of a word as Metrics::record reads it: an initialisation error is a series of its
// own; a bypassed request counts as accepted, not mutated, without an error code (service.rs:45-58);
// else the vanilla response's bits, and error code 500 for a group expression that failed.
KW_HD inline uint32_t outcome_code(uint32_t w) {
  if (((w & KW_F_STATUS_MASK) >> KW_F_STATUS_SHIFT) == (uint32_t)KW_FST_INIT_ERROR) return (uint32_t)KW_OUT_INIT_ERROR;
  if (w & KW_BYPASS) return (uint32_t)KW_OUT_ACCEPTED;
  return (w & (KW_V_ALLOWED | KW_V_MUTATED)) | (KW_REASON(w) == (uint32_t)KW_R_GROUP_EXPR ? (uint32_t)KW_OUT_ERROR_500 : 0u);
}
static_assert(KW_OUT_ACCEPTED == KW_V_ALLOWED && KW_OUT_MUTATED == KW_V_MUTATED && KW_OUT_ERROR_500 == 4 &&
                  KW_OUT_INIT_ERROR == 8 && KW_OUT_N == 9,
              "kw_outcome layout");

inline size_t outcome_table_words(uint32_t ngroups, uint32_t npol) { return (size_t)ngroups * KW_OUT_N * npol; }

// The reference reducer: words [rows][npol] with row_group[rows] (nullptr: one group) into
// out[ngroups][KW_OUT_N][npol]. The column is innermost: the device's adds of one outcome are
// contiguous.
inline int outcome_reduce(const uint32_t* words, uint64_t rows, uint32_t npol, const uint32_t* row_group, uint32_t ngroups,
                          uint64_t* out) {
  if (!out || npol == 0 || ngroups == 0 || (rows && !words)) return KW_E_ARG;
  for (uint64_t r = 0; r < rows; ++r)
    if (row_group && row_group[r] >= ngroups) return KW_E_ARG;
  for (size_t i = 0; i < outcome_table_words(ngroups, npol); ++i) out[i] = 0;
  for (uint64_t r = 0; r < rows; ++r) {
    uint64_t* t = out + (size_t)(row_group ? row_group[r] : 0u) * KW_OUT_N * npol;
    for (uint32_t c = 0; c < npol; ++c) t[(size_t)outcome_code(words[r * npol + c]) * npol + c] += 1u;
  }
  return KW_OK;
}

// ---- the count kernel's geometry ----
// The rows are sorted by group (a counting sort, stable: each group keeps batch order), so a group
// is one run of the sorted list and a range of consecutive groups one slice of it. A unit is one
// group's run of at most kOutUnitRows consecutive entries; a wave counts one unit in registers and
// adds its non-zero counters to the table once.
constexpr uint32_t kOutUnitRows = 256;  // R: entries of a unit
constexpr uint32_t kOutWaves = 4;       // waves of a workgroup (256 threads), a unit each
constexpr uint32_t kOutLoads = 16;      // row loads a lane keeps in flight

struct OutUnit {
  uint32_t first;  // index of the unit's first entry in the sorted list
  uint32_t n;      // its entries, 1..kOutUnitRows
  uint32_t group;
};

// start[g] = the first sorted index of group g (start[ngroups] = rows); order[i] = the row at
// sorted index i. row_group nullptr: one group. False when an id is >= ngroups (nothing usable
// written). rows < 2^32.
inline bool outcome_sort(const uint32_t* row_group, uint64_t rows, uint32_t ngroups, uint32_t* start, uint32_t* order) {
  for (uint32_t g = 0; g <= ngroups; ++g) start[g] = 0;
  for (uint64_t r = 0; r < rows; ++r) {
    const uint32_t g = row_group ? row_group[r] : 0u;
    if (g >= ngroups) return false;
    ++start[g + 1];
  }
  for (uint32_t g = 0; g < ngroups; ++g) start[g + 1] += start[g];
  // (start[g] serves as group g's cursor and is shifted back afterwards)
  for (uint64_t r = 0; r < rows; ++r) order[start[row_group ? row_group[r] : 0u]++] = (uint32_t)r;
  for (uint32_t g = ngroups; g > 0; --g) start[g] = start[g - 1];
  start[0] = 0;
  return true;
}

// The units of groups [g0, g1): their number, and the table itself (u holds that many).
inline uint64_t outcome_unit_count(const uint32_t* start, uint32_t g0, uint32_t g1) {
  uint64_t n = 0;
  for (uint32_t g = g0; g < g1; ++g) n += ((uint64_t)(start[g + 1] - start[g]) + kOutUnitRows - 1u) / kOutUnitRows;
  return n;
}
inline void outcome_fill_units(const uint32_t* start, uint32_t g0, uint32_t g1, OutUnit* u) {
  for (uint32_t g = g0; g < g1; ++g)
    for (uint32_t s = start[g]; s < start[g + 1]; s += kOutUnitRows) {
      const uint32_t left = start[g + 1] - s;
      *u++ = OutUnit{s, left < kOutUnitRows ? left : kOutUnitRows, g};
      if (left <= kOutUnitRows) break;  // (s + kOutUnitRows may wrap at the end of a 2^32-row list)
    }
}

// The groups of one range under a table budget of `bytes`: range k holds the groups
// [k * q, min(ngroups, (k + 1) * q)). A budget below one group's counters still takes one group.
inline uint32_t outcome_range_groups(uint32_t npol, uint64_t bytes) {
  const uint64_t per = (uint64_t)KW_OUT_N * npol * sizeof(uint64_t), q = bytes / (per ? per : 1u);
  return q < 1u ? 1u : q > 0xffffffffull ? 0xffffffffu : (uint32_t)q;
}
inline uint32_t outcome_ranges(uint32_t ngroups, uint32_t per_range) { return (ngroups + per_range - 1u) / per_range; }

// What `lane` of the wave that counts a unit of n entries reads in round t (pack_geom's w lanes a
// row, ipi rows a load): entry t * ipi + lane / w of the unit, column 64 grp + lane % w.
struct OutLane {
  uint32_t entry, col;
  bool on;
};
KW_HD inline OutLane out_lane(const PackGeom& p, uint32_t npol, uint32_t grp, uint32_t n, uint32_t t, uint32_t lane) {
  OutLane L;
  const uint32_t sub = lane / p.w;
  L.entry = t * p.ipi + sub;
  L.col = 64u * grp + lane % p.w;
  L.on = sub < p.ipi && L.entry < n && L.col < npol;
  return L;
}
KW_HD inline uint32_t out_rounds(const PackGeom& p, uint32_t n) { return (n + p.ipi - 1u) / p.ipi; }

}  // namespace kw
