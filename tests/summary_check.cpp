// summary_check — the summary form (include/kwgpu.h kw_summary, policy-server_amd/csrc/summary.hpp)
// on the host, no GPU and no Python in the process (tests/test_summary.py builds it with
// -fsanitize=address,undefined and runs it). Header only: the reference reducer on every pair of a
// small synthetic pass against counters and bits worked out here, and the reduction kernel's
// geometry (sum_geom, sum_lane) walked the way the kernel walks it: every (row, column) is covered
// exactly once and a plane slot is stored once, over npol 1..300 and rows 0, 1, 63, 64, 65; the grid
// and the per-workgroup row cap at rows = 2^40 as well.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "summary.hpp"

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

// A word with every field drawn from the generator: a product reason 0..15, or now and then the
// poison sentinel.
static uint32_t rnd_word(uint64_t* s) {
  *s = *s * 6364136223846793005ull + 1442695040888963407ull;
  const uint32_t x = (uint32_t)(*s >> 32);
  if (x % 97u == 0) return 0xA5A5A5A5u;
  const uint32_t reason = (x >> 8) % 16u, flags = x & 0x7fu;
  return flags | (reason << 8) | (x & 0xffff0000u);
}

static void check_reducer(uint64_t rows, uint32_t npol, bool with_planes) {
  ++cases;
  const uint32_t G = kw::packed_groups(npol);
  uint64_t seed = rows * 1000003u + npol;
  std::vector<uint32_t> w(rows * npol);
  for (uint32_t& x : w) x = rnd_word(&seed);
  std::vector<uint64_t> col((size_t)npol * KW_SUM_N, ~0ull), planes((size_t)rows * G * 2, ~0ull);
  kw_summary s{rows, npol, col.data(), with_planes ? planes.data() : nullptr};
  const int rc = kw::summary_reduce(w.data(), &s);
  CHECK(rc == KW_OK, "reduce rows %llu npol %u: rc %d", (unsigned long long)rows, npol, rc);
  // every pair, by the definitions of include/kwgpu.h written out here
  std::vector<uint64_t> want((size_t)npol * KW_SUM_N, 0);
  size_t bad_bits = 0;
  for (uint64_t r = 0; r < rows; ++r)
    for (uint32_t c = 0; c < npol; ++c) {
      const uint32_t x = w[r * npol + c], reason = (x >> 8) & 0xffu, st = (x >> 3) & 3u;
      uint64_t* k = &want[(size_t)c * KW_SUM_N];
      k[KW_SUM_F_ALLOWED] += (x >> 2) & 1u;
      k[KW_SUM_V_ALLOWED] += x & 1u;
      k[KW_SUM_V_MUTATED] += (x >> 1) & 1u;
      k[KW_SUM_F_PATCH] += (x >> 6) & 1u;
      k[KW_SUM_BYPASS] += (x >> 5) & 1u;
      if (st == 1) ++k[KW_SUM_FST_VANILLA];
      if (st == 2) ++k[KW_SUM_FST_MUTATION_REFUSED];
      if (st == 3) ++k[KW_SUM_FST_INIT_ERROR];
      ++k[reason <= 15 ? (uint32_t)KW_SUM_REASON + reason : (uint32_t)KW_SUM_REASON_OTHER];
      if (with_planes) {
        const uint64_t p0 = planes[2 * (r * G + c / 64)], p1 = planes[2 * (r * G + c / 64) + 1];
        bad_bits += ((p0 >> (c % 64)) & 1u) != (reason > 15 ? 1u : ((x >> 2) & 1u) ^ 1u);  // (an "other" word: both bits)
        bad_bits += ((p1 >> (c % 64)) & 1u) != (reason ? 1u : 0u);
      }
    }
  CHECK(col == want, "reduce rows %llu npol %u: counters differ", (unsigned long long)rows, npol);
  CHECK(bad_bits == 0, "reduce rows %llu npol %u: %zu plane bits differ", (unsigned long long)rows, npol, bad_bits);
  if (with_planes && npol % 64)
    for (uint64_t r = 0; r < rows; ++r)
      for (int h = 0; h < 2; ++h)
        CHECK((planes[2 * (r * G + G - 1) + h] >> (npol % 64)) == 0, "padding bits set in row %llu", (unsigned long long)r);
  for (uint32_t c = 0; c < npol; ++c)
    for (uint32_t k = 9; k < 16; ++k) CHECK(col[(size_t)c * KW_SUM_N + k] == 0, "counter %u of column %u is not zero", k, c);
}

// The kernel's walk: workgroup (x, grp), wave, the units wave strides to, rounds, lanes.
static void check_geometry(uint64_t rows, uint32_t npol, uint32_t ncu) {
  ++cases;
  const kw::SumGeom g = kw::sum_geom(rows, npol, ncu);
  const uint32_t G = kw::packed_groups(npol);
  CHECK(g.G == G && g.grid_x >= 1 && g.cols == g.p.w && g.p.T <= kw::kSumRounds && g.p.ipw <= 64, "geometry npol %u", npol);
  CHECK(kw::sum_wg_rows(g) < (1ull << 32), "rows %llu npol %u: a workgroup counts %llu rows", (unsigned long long)rows, npol,
        (unsigned long long)kw::sum_wg_rows(g));
  CHECK((uint64_t)g.units * g.p.ipw >= rows && (g.units == 0 || (g.units - 1) * g.p.ipw < rows), "rows %llu npol %u: units",
        (unsigned long long)rows, npol);
  if (rows > 4096) return;  // (the walk itself only at sizes a test can enumerate)
  std::vector<uint8_t> seen(rows * npol, 0), stored(rows * G, 0);
  const uint64_t nwaves = (uint64_t)kw::kSumWaves * g.grid_x;
  size_t out_of_range = 0, moved = 0;
  for (uint32_t grp = 0; grp < G; ++grp)
    for (uint64_t wave = 0; wave < nwaves; ++wave) {
      uint32_t lane_col[64];
      for (uint32_t lane = 0; lane < 64; ++lane) lane_col[lane] = ~0u;
      uint64_t wave_rows = 0;
      for (uint64_t unit = wave; unit < g.units; unit += nwaves) {
        for (uint32_t t = 0; t < kw::kSumRounds; ++t)
          for (uint32_t lane = 0; lane < 64; ++lane) {
            const kw::SumLane L = kw::sum_lane(g, rows, npol, grp, unit, t, lane);
            if (!L.on) continue;
            if (L.row >= rows || L.col >= npol || L.c >= g.cols) {
              ++out_of_range;
              continue;
            }
            ++seen[L.row * npol + L.col];
            if (lane_col[lane] != ~0u && lane_col[lane] != L.col) ++moved;  // a lane keeps one column
            lane_col[lane] = L.col;
            if (lane == 0) ++wave_rows;
          }
        for (uint32_t lane = 0; lane < g.p.ipw; ++lane)  // the unit's plane stores
          if (unit * g.p.ipw + lane < rows) ++stored[(unit * g.p.ipw + lane) * G + grp];
      }
      CHECK(wave_rows <= kw::sum_wg_rows(g), "a lane saw more rows than the cap");
    }
  size_t bad = 0, bad_store = 0;
  for (uint8_t v : seen) bad += v != 1;
  for (uint8_t v : stored) bad_store += v != 1;
  CHECK(out_of_range == 0 && moved == 0, "rows %llu npol %u: %zu out of range, %zu lanes changed column", (unsigned long long)rows,
        npol, out_of_range, moved);
  CHECK(bad == 0, "rows %llu npol %u ncu %u: %zu pairs not covered exactly once", (unsigned long long)rows, npol, ncu, bad);
  CHECK(bad_store == 0, "rows %llu npol %u: %zu plane slots not stored exactly once", (unsigned long long)rows, npol, bad_store);
}

int main() {
  for (uint32_t npol : {1u, 3u, 4u, 31u, 32u, 33u, 63u, 64u, 65u, 128u, 130u})
    for (uint64_t rows : {0ull, 1ull, 2ull, 63ull, 64ull, 65ull, 300ull})
      for (bool planes : {true, false}) check_reducer(rows, npol, planes);
  // the poison word alone: the "other" bucket and both planes
  {
    ++cases;
    const uint32_t w = 0xA5A5A5A5u;
    uint64_t col[KW_SUM_N], pl[2];
    kw_summary s{1, 1, col, pl};
    CHECK(kw::summary_reduce(&w, &s) == KW_OK && col[KW_SUM_REASON_OTHER] == 1 && pl[0] == 1 && pl[1] == 1, "poison word");
    uint64_t sum = 0;
    for (int k = KW_SUM_REASON; k < KW_SUM_N; ++k) sum += col[k];
    CHECK(sum == 0, "poison word counted in a product reason");
    kw_summary bad{1, 0, col, pl};
    CHECK(kw::summary_reduce(&w, &bad) == KW_E_ARG, "npol 0");
  }
  for (uint32_t npol = 1; npol <= 300; ++npol)
    for (uint64_t rows : {0ull, 1ull, 63ull, 64ull, 65ull, 1ull << 40})
      for (uint32_t ncu : {0u, 1u, 256u}) check_geometry(rows, npol, ncu);
  // several units per wave: a device of one unit keeps the grid at two workgroups
  for (uint32_t npol : {1u, 5u, 32u, 64u, 70u}) check_geometry(3001, npol, 1);
  printf("cases %d failures %d\n", cases, failures);
  return failures ? 1 : 0;
}
