// outcomes_check — the grouped outcome count (include/kwgpu.h kw_batch_outcomes,
// policy-server_amd/csrc/outcomes.hpp) on the host, no GPU and no Python in the process
// (tests/test_outcomes.py builds it with -fsanitize=address,undefined and runs it). Header only: the
// counting sort is a stable permutation, the units never cross a group and never exceed R, every
// sorted entry lies in exactly one unit, the range cut covers every group once within its budget;
// the kernel's lane geometry (out_lane) walked the way the kernel walks it covers every (entry,
// column) of a unit exactly once; the reference reducer against counters worked out here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "outcomes.hpp"

static int failures = 0, cases = 0;
#define CHECK(c, ...)                              \
  do {                                             \
    if (!(c)) {                                    \
      if (++failures <= 20) {                      \
        fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);              \
        fprintf(stderr, "\n");                     \
      }                                            \
    }                                              \
  } while (0)

using kw::kOutUnitRows;
using kw::OutUnit;

// The geometry over one assignment of rows to groups, for each table budget.
static void check_groups(const char* what, const std::vector<uint32_t>& row_group, uint32_t ngroups, bool one_group_null = false) {
  ++cases;
  const uint64_t rows = row_group.size();
  // exact-size blocks: an access one past any of them is the sanitizer's to catch
  std::vector<uint32_t> start((size_t)ngroups + 1, 0xdeadbeefu), order((size_t)rows, 0xdeadbeefu);
  const bool ok = kw::outcome_sort(one_group_null ? nullptr : row_group.data(), rows, ngroups, start.data(), order.data());
  CHECK(ok, "%s: sort refused valid ids", what);
  if (!ok) return;
  CHECK(start[0] == 0 && start[ngroups] == rows, "%s: start[0] %u start[n] %u rows %llu", what, start[0], start[ngroups],
        (unsigned long long)rows);
  // a permutation, each group's slice holding exactly its rows in batch order
  std::vector<uint8_t> seen((size_t)rows, 0);
  size_t bad = 0;
  for (uint32_t g = 0; g < ngroups; ++g) {
    CHECK(start[g] <= start[g + 1], "%s: start not monotonic at %u", what, g);
    for (uint32_t i = start[g]; i < start[g + 1]; ++i) {
      const uint32_t r = order[i];
      if (r >= rows || seen[r] || row_group[r] != g || (i > start[g] && order[i - 1] >= r)) ++bad;
      if (r < rows) seen[r] = 1;
    }
  }
  CHECK(bad == 0, "%s: %zu sorted entries out of place (not a stable permutation)", what, bad);
  // the units of all groups
  const uint64_t nunits = kw::outcome_unit_count(start.data(), 0, ngroups);
  std::vector<OutUnit> units((size_t)nunits);
  kw::outcome_fill_units(start.data(), 0, ngroups, units.data());
  std::vector<uint32_t> covered((size_t)rows, 0);
  bad = 0;
  for (const OutUnit& u : units) {
    if (u.n == 0 || u.n > kOutUnitRows || u.group >= ngroups || u.first < start[u.group] ||
        (uint64_t)u.first + u.n > start[u.group + 1]) {
      ++bad;
      continue;
    }
    for (uint32_t i = 0; i < u.n; ++i) ++covered[u.first + i];
  }
  CHECK(bad == 0, "%s: %zu units cross a group or exceed R", what, bad);
  bad = 0;
  for (uint32_t c : covered) bad += c != 1;
  CHECK(bad == 0, "%s: %zu sorted entries not in exactly one unit", what, bad);
  // no more units than needed: a group of n rows takes ceil(n / R)
  uint64_t least = 0;
  for (uint32_t g = 0; g < ngroups; ++g) least += ((uint64_t)(start[g + 1] - start[g]) + kOutUnitRows - 1) / kOutUnitRows;
  CHECK(nunits == least, "%s: %llu units, %llu needed", what, (unsigned long long)nunits, (unsigned long long)least);
  // the range cut under several budgets: every group in one range, each range within the budget, and
  // the ranges' unit tables together the whole one
  for (uint32_t npol : {1u, 64u, 65u})
    for (uint64_t budget : {72ull * npol, 72ull * npol * 3 + 5, 1ull << 20, 64ull << 20}) {
      const uint32_t per = kw::outcome_range_groups(npol, budget), nr = kw::outcome_ranges(ngroups, per);
      CHECK(per >= 1 && (uint64_t)per * KW_OUT_N * npol * 8 <= budget, "%s: %u groups a range over budget %llu", what, per,
            (unsigned long long)budget);
      std::vector<uint32_t> in((size_t)ngroups, 0);
      uint64_t at = 0;
      for (uint32_t k = 0; k < nr; ++k) {
        const uint32_t g0 = k * per, g1 = (uint64_t)(k + 1) * per < ngroups ? (k + 1) * per : ngroups;
        CHECK(g0 < g1, "%s: empty range %u", what, k);
        for (uint32_t g = g0; g < g1; ++g) ++in[g];
        CHECK(kw::outcome_table_words(g1 - g0, npol) * 8 <= budget, "%s: range %u over budget", what, k);
        const uint64_t n = kw::outcome_unit_count(start.data(), g0, g1);
        std::vector<OutUnit> part((size_t)n);
        kw::outcome_fill_units(start.data(), g0, g1, part.data());
        CHECK(at + n <= nunits && (n == 0 || memcmp(part.data(), units.data() + at, n * sizeof(OutUnit)) == 0),
              "%s: range %u's units are not its slice of the table", what, k);
        at += n;
      }
      bad = 0;
      for (uint32_t c : in) bad += c != 1;
      CHECK(bad == 0 && at == nunits, "%s: %zu groups not in exactly one range", what, bad);
    }
  CHECK(kw::outcome_range_groups(64, 1) == 1, "a budget below one group still takes one group");
}

// The lanes of a wave over a unit of n entries: every (entry, column) of column group grp read once.
static void check_lanes(uint32_t npol, uint32_t n) {
  ++cases;
  const kw::PackGeom p = kw::pack_geom(npol);
  const uint32_t G = kw::packed_groups(npol), rounds = kw::out_rounds(p, n);
  std::vector<uint32_t> hit((size_t)n * npol, 0);
  size_t out_of_range = 0;
  for (uint32_t grp = 0; grp < G; ++grp)
    // (the kernel runs its rounds in batches of kOutLoads: the rounds past the last are all off)
    for (uint32_t t = 0; t < (rounds + kw::kOutLoads - 1) / kw::kOutLoads * kw::kOutLoads; ++t)
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const kw::OutLane L = kw::out_lane(p, npol, grp, n, t, lane);
        if (!L.on) continue;
        if (L.entry >= n || L.col >= npol || t >= rounds) ++out_of_range;
        else ++hit[(size_t)L.entry * npol + L.col];
        // the lane that sums this column's sub-rows is lane % w, below w * ipi <= 64
        if (lane % p.w + (p.ipi - 1) * p.w > 63) ++out_of_range;
      }
  size_t bad = 0;
  for (uint32_t h : hit) bad += h != 1;
  CHECK(out_of_range == 0 && bad == 0, "npol %u n %u: %zu out of range, %zu pairs not read exactly once", npol, n, out_of_range, bad);
}

static uint32_t rnd(uint64_t* s) {
  *s = *s * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(*s >> 32);
}

static void check_reducer(uint64_t rows, uint32_t npol, uint32_t ngroups) {
  ++cases;
  uint64_t seed = rows * 1000003u + npol * 31u + ngroups;
  std::vector<uint32_t> w((size_t)rows * npol), rg((size_t)rows);
  for (uint32_t& x : w) {
    const uint32_t r = rnd(&seed);
    x = r % 97u == 0 ? 0xA5A5A5A5u : ((r & 0x7fu) | (((r >> 8) % 16u) << 8) | (r & 0xffff0000u));
  }
  for (uint32_t& g : rg) g = rnd(&seed) % ngroups;
  std::vector<uint64_t> out(kw::outcome_table_words(ngroups, npol), ~0ull), want(out.size(), 0);
  CHECK(kw::outcome_reduce(w.data(), rows, npol, rg.data(), ngroups, out.data()) == KW_OK, "reduce failed");
  for (uint64_t r = 0; r < rows; ++r)
    for (uint32_t c = 0; c < npol; ++c) {
      // Metrics::record written out: init error; else bypass -> accepted; else the vanilla bits and 500
      const uint32_t x = w[r * npol + c];
      uint32_t k;
      if (((x >> 3) & 3u) == 3u) k = 8;
      else if (x & 0x20u) k = 1;
      else k = (x & 1u) | (x & 2u) | ((((x >> 8) & 0xffu) == 14u) ? 4u : 0u);
      ++want[((size_t)rg[r] * KW_OUT_N + k) * npol + c];
    }
  CHECK(out == want, "reducer rows %llu npol %u groups %u differs", (unsigned long long)rows, npol, ngroups);
  if (rows) {
    rg[rows / 2] = ngroups;  // an id out of range: refused, by the reducer and by the sort
    CHECK(kw::outcome_reduce(w.data(), rows, npol, rg.data(), ngroups, out.data()) == KW_E_ARG, "id >= ngroups accepted");
    std::vector<uint32_t> start((size_t)ngroups + 1), order((size_t)rows);
    CHECK(!kw::outcome_sort(rg.data(), rows, ngroups, start.data(), order.data()), "sort accepted id >= ngroups");
  }
}

int main() {
  const uint32_t R = kOutUnitRows;
  check_groups("0 rows", {}, 1);
  check_groups("0 rows, 5 groups", {}, 5);
  check_groups("1 row", {0}, 1);
  check_groups("1 row in the last of 4 groups", {3}, 4);
  for (uint32_t n : {R - 1, R, R + 1, 2 * R + 1}) {
    char what[64];
    snprintf(what, sizeof what, "one group of %u", n);
    check_groups(what, std::vector<uint32_t>(n, 0), 1);
    check_groups(what, std::vector<uint32_t>(n, 0), 1, true);  // row_group == nullptr
    // the same group between two others, interleaved with them
    std::vector<uint32_t> mix;
    for (uint32_t i = 0; i < n; ++i) {
      mix.push_back(1);
      if (i % 3 == 0) mix.push_back(i % 2 ? 0 : 2);
    }
    snprintf(what, sizeof what, "group of %u interleaved", n);
    check_groups(what, mix, 3);
  }
  {
    std::vector<uint32_t> own(1000);
    for (uint32_t i = 0; i < own.size(); ++i) own[i] = (uint32_t)own.size() - 1 - i;  // ngroups == rows, reversed
    check_groups("every row its own group", own, (uint32_t)own.size());
    std::vector<uint32_t> holes;
    for (uint32_t i = 0; i < 3000; ++i) holes.push_back(i % 7 == 0 ? 0 : i % 7 == 1 ? 5 : 2);  // 1, 3, 4 and 6..9 empty
    check_groups("empty groups in the middle and at the end", holes, 10);
    uint64_t seed = 12345;
    std::vector<uint32_t> any(5000);
    for (uint32_t& g : any) g = rnd(&seed) % 37u;
    check_groups("random ids", any, 37);
  }
  for (uint32_t npol : {1u, 2u, 3u, 31u, 32u, 33u, 63u, 64u, 65u, 128u, 130u})
    for (uint32_t n : {1u, 2u, 15u, 16u, 17u, R - 1, R}) check_lanes(npol, n);
  for (uint32_t npol : {1u, 31u, 64u, 65u})
    for (uint64_t rows : {0ull, 1ull, 300ull})
      for (uint32_t ng : {1u, 7u}) check_reducer(rows, npol, ng);
  // all nine codes by hand, a bypass word with V_MUTATED set, the poison word
  {
    ++cases;
    const uint32_t ge = 14u << 8;
    const uint32_t w[12] = {0, 1, 2, 3, ge, ge | 1, ge | 2, ge | 3, 3u << 3, 0x20u | 2u, 0x20u | ge, 0xA5A5A5A5u};
    const uint32_t want[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 1, 1, 1};  // (the poison word has BYPASS set, F_STATUS 0)
    for (int i = 0; i < 12; ++i) CHECK(kw::outcome_code(w[i]) == want[i], "word %08x: code %u", w[i], kw::outcome_code(w[i]));
  }
  printf("cases %d failures %d\n", cases, failures);
  return failures ? 1 : 0;
}
