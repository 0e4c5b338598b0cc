// summary.hpp — the pure arithmetic of the summary form (include/kwgpu.h kw_summary): per-column
// counters of a pass's verdict words and two bit-planes per 64-column group that mark the pairs worth
// a message. The bucket and bit functions, the reference host reducer, and the geometry of the
// reduction kernels (reports.hip summary_kernel): which (row, column) a lane reads in which round,
// the grid, and the cap that keeps the u32 partial counters from wrapping. The device kernels share
// all of it. No HIP, no batch, no settings (tests/summary_check.cpp runs it on the host).
//
// What the counters replace: the accepted / mutated / error counts of
// kubewarden_policy_evaluations_total (src/metrics.rs:49-140) per policy are col[c][KW_SUM_V_ALLOWED],
// [KW_SUM_V_MUTATED] and [KW_SUM_FST_INIT_ERROR] / [KW_SUM_REASON + r]; the attribute sets with the
// per-request kind / operation / namespace are counted by kw_batch_outcomes (outcomes.hpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "packed.hpp"
#include "slots.hpp"

namespace kw {

// The reason bucket of a word: KW_SUM_REASON + its reason, or KW_SUM_REASON_OTHER for a reason no
// product word carries (the poison sentinel 0xA5A5A5A5 has reason 0xA5).
static_assert(KW_R_INIT_ERROR == 15, "the reason buckets KW_SUM_REASON + 0..15 hold every kw_reason");
static_assert(KW_SUM_REASON + KW_R_INIT_ERROR < KW_SUM_N && KW_SUM_REASON_OTHER < KW_SUM_REASON, "kw_summary layout");
KW_HD inline uint32_t sum_reason_bucket(uint32_t w) {
  const uint32_t r = KW_REASON(w);
  return r <= 15u ? (uint32_t)KW_SUM_REASON + r : (uint32_t)KW_SUM_REASON_OTHER;
}
// The F_STATUS bucket of a word (KW_SUM_FST_*), or KW_SUM_N for status None (not counted).
KW_HD inline uint32_t sum_status_bucket(uint32_t w) {
  const uint32_t st = (w & KW_F_STATUS_MASK) >> KW_F_STATUS_SHIFT;
  return st ? (uint32_t)KW_SUM_FST_VANILLA + st - 1u : (uint32_t)KW_SUM_N;
}
static_assert(KW_SUM_FST_VANILLA + KW_FST_INIT_ERROR - 1 == KW_SUM_FST_INIT_ERROR, "status buckets follow KW_FST_*");
// The plane bits of a word: the final answer is a reject; the policy found something. A word of the
// "other" bucket is no product word and none of its bits means anything (the poison sentinel happens
// to have KW_F_ALLOWED set): it sets both bits, so a pair that was never evaluated is always flagged.
KW_HD inline uint32_t sum_bit_reject(uint32_t w) { return (w & KW_F_ALLOWED) && KW_REASON(w) <= 15u ? 0u : 1u; }
KW_HD inline uint32_t sum_bit_found(uint32_t w) { return KW_REASON(w) ? 1u : 0u; }

// One word into a column's counters (c: KW_SUM_N of them).
template <typename T>
KW_HD inline void sum_count_word(uint32_t w, T* c) {
  c[KW_SUM_F_ALLOWED] += (w & KW_F_ALLOWED) ? 1u : 0u;
  c[KW_SUM_V_ALLOWED] += (w & KW_V_ALLOWED) ? 1u : 0u;
  c[KW_SUM_V_MUTATED] += (w & KW_V_MUTATED) ? 1u : 0u;
  c[KW_SUM_F_PATCH] += (w & KW_F_PATCH) ? 1u : 0u;
  c[KW_SUM_BYPASS] += (w & KW_BYPASS) ? 1u : 0u;
  const uint32_t st = sum_status_bucket(w);
  if (st < (uint32_t)KW_SUM_N) c[st] += 1u;
  c[sum_reason_bucket(w)] += 1u;
}

inline size_t summary_col_words(uint32_t npol) { return (size_t)npol * KW_SUM_N; }

// The reference reducer: words [rows][npol] into s->col and, when given, s->planes.
inline int summary_reduce(const uint32_t* words, kw_summary* s) {
  if (!s || s->npol == 0 || !s->col || (s->rows && !words)) return KW_E_ARG;
  const uint32_t npol = s->npol, G = packed_groups(npol);
  for (size_t i = 0; i < summary_col_words(npol); ++i) s->col[i] = 0;
  for (uint64_t r = 0; r < s->rows; ++r)
    for (uint32_t g = 0; g < G; ++g) {
      uint64_t rej = 0, found = 0;
      for (uint32_t c = 0; c < 64u && 64u * g + c < npol; ++c) {
        const uint32_t col = 64u * g + c, w = words[r * npol + col];
        sum_count_word(w, s->col + (size_t)col * KW_SUM_N);
        rej |= (uint64_t)sum_bit_reject(w) << c;
        found |= (uint64_t)sum_bit_found(w) << c;
      }
      if (s->planes) {
        s->planes[2 * (r * G + g)] = rej;
        s->planes[2 * (r * G + g) + 1] = found;
      }
    }
  return KW_OK;
}

// ---- the reduction kernel's geometry ----
// A lane keeps one column for the whole kernel. The lanes of a wave cover rows as the pack kernels'
// do (packed.hpp pack_geom): a row takes w lanes (64, or npol where npol <= 32, and a wave then takes
// ipi = 64 / npol rows a round); T rounds make a unit of ipw = ipi * T consecutive rows, after which
// lane j < ipw holds row j's two plane words. A wave is bound to one column group (grid.y = G) and
// takes the units wave, wave + W, wave + 2 W, ... of the W = kSumWaves * grid_x waves of its group.
// Each workgroup writes one u32 partial block [cols][KW_SUM_N] at part[(group * grid_x + x)].
constexpr uint32_t kSumWaves = 4;           // waves of a workgroup (256 threads)
constexpr uint32_t kSumRounds = 16;         // the most rounds of a unit (pack_geom's T <= 16)
constexpr uint64_t kSumWgRows = 1ull << 30;  // rows one workgroup may count (a u32 counter holds 4 x that)
struct SumGeom {
  PackGeom p;
  uint32_t G;       // column groups
  uint32_t cols;    // columns of a workgroup's partial block: p.w
  uint64_t units;   // units of p.ipw rows
  uint32_t grid_x;  // workgroups per column group
};
// The geometry of a launch over rows x npol on a device of ncu compute units (0: 256): about two
// workgroups per unit over all groups, fewer where the rows are few, more where a workgroup would
// otherwise count more than kSumWgRows rows.
KW_HD inline SumGeom sum_geom(uint64_t rows, uint32_t npol, uint32_t ncu) {
  SumGeom g;
  g.p = pack_geom(npol);
  g.G = packed_groups(npol);
  g.cols = g.p.w;
  g.units = (rows + g.p.ipw - 1u) / g.p.ipw;
  const uint64_t want = (g.units + kSumWaves - 1u) / kSumWaves;
  const uint64_t fill = 2ull * (ncu ? ncu : 256u) / g.G;
  const uint64_t least = (rows + kSumWgRows - 1u) / kSumWgRows;
  uint64_t x = want < fill ? want : fill;
  if (x < least) x = least;
  g.grid_x = (uint32_t)(x ? x : 1u);
  return g;
}
// The most rows whose words one workgroup adds into one u32 counter (the cap: < 2^32).
KW_HD inline uint64_t sum_wg_rows(const SumGeom& g) {
  const uint64_t waves = (uint64_t)kSumWaves * g.grid_x;
  return (uint64_t)kSumWaves * ((g.units + waves - 1u) / waves) * g.p.ipw;
}
KW_HD inline uint64_t sum_part_words(const SumGeom& g) { return (uint64_t)g.G * g.grid_x * g.cols * KW_SUM_N; }

// What `lane` of the wave that runs `unit` of column group `grp` holds in round t.
struct SumLane {
  uint64_t row;
  uint32_t col, c;
  bool on;
};
KW_HD inline SumLane sum_lane(const SumGeom& g, uint64_t rows, uint32_t npol, uint32_t grp, uint64_t unit, uint32_t t,
                              uint32_t lane) {
  SumLane L;
  const uint32_t sub = lane / g.p.w;
  L.c = lane % g.p.w;
  L.row = unit * g.p.ipw + (uint64_t)t * g.p.ipi + sub;
  L.col = 64u * grp + L.c;
  L.on = t < g.p.T && sub < g.p.ipi && L.row < rows && L.col < npol;
  return L;
}

}  // namespace kw
