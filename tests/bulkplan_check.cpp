// Host check of the bulk path's arithmetic (policy-server_amd/csrc/bulkplan.hpp, the header
// bulk.cpp runs): the chunk schedule against boundaries recorded from the loop it replaced
// (tests/golden/bulk_chunks.txt, one case a line: ntiles tile_rows per_rows ramp : b0 b1 ...) and
// against its properties, the slab schedule of an unchunked pass, and the packed placement of a
// chunk's ranges against the slot-size estimate that has to cover it.
// Built and run by tests/test_bulkplan.py:  g++ -O2 -std=c++17 -I policy-server_amd/csrc
#include <cstdio>
#include <cstdlib>

#include "bulkplan.hpp"

using namespace kw;

static int bad = 0;
#define CHECK(c, ...)                  \
  do {                                 \
    if (!(c)) {                        \
      if (++bad <= 20) {               \
        fprintf(stderr, "FAIL %s: ", #c); \
        fprintf(stderr, __VA_ARGS__);  \
        fprintf(stderr, "\n");         \
      }                                \
    }                                  \
  } while (0)

static void check_chunks(uint64_t ntiles, uint64_t rows, uint64_t per, bool ramp, const std::vector<uint64_t>& want) {
  const std::vector<uint64_t> tb = chunk_bounds(ntiles, rows, per, ramp);
  const unsigned long long a = ntiles, b = rows, c = per;
  CHECK(tb == want, "%llu %llu %llu %d: boundaries differ from the recorded ones", a, b, c, (int)ramp);
  const uint64_t tper = std::max<uint64_t>({1, per / rows, (ntiles + 239) / 240});
  CHECK(chunk_tiles(ntiles, rows, per) == tper, "%llu %llu %llu", a, b, c);
  CHECK(tb.size() >= 2 && tb.front() == 0 && tb.back() == ntiles, "%llu %llu %llu %d: ends", a, b, c, (int)ramp);
  for (size_t k = 0; k + 1 < tb.size(); ++k) {
    CHECK(tb[k] < tb[k + 1], "%llu %llu %llu %d: chunk %zu empty", a, b, c, (int)ramp, k);
    CHECK(tb[k + 1] - tb[k] <= tper, "%llu %llu %llu %d: chunk %zu above tper", a, b, c, (int)ramp, k);
    if (!ramp && k + 2 < tb.size()) CHECK(tb[k + 1] - tb[k] == tper, "%llu %llu %llu: chunk %zu not tper", a, b, c, k);
  }
  if (ramp && tb.size() >= 2)
    CHECK(tb[1] == std::min(ntiles, std::max<uint64_t>(1, tper / 16)), "%llu %llu %llu: first chunk", a, b, c);
}

// The slab schedule of an unchunked pass: its properties, and `want` where the bounds are given.
static void check_slabs(uint64_t rows, uint64_t per, const std::vector<uint64_t>* want = nullptr) {
  const std::vector<uint64_t> rb = slab_bounds(rows, per);
  const unsigned long long a = rows, b = per;
  if (want) CHECK(rb == *want, "slabs %llu %llu: bounds differ from the given ones", a, b);
  const uint64_t slab = std::max<uint64_t>({1, per, (rows + 239) / 240});
  CHECK(!rb.empty() && rb.front() == 0 && rb.back() == rows, "slabs %llu %llu: ends", a, b);
  CHECK(rb.size() == (rows + slab - 1) / slab + 1, "slabs %llu %llu: %zu bounds", a, b, rb.size());
  CHECK(rb.size() - 1 <= 240, "slabs %llu %llu: %zu slabs", a, b, rb.size() - 1);  // (per above ceil(rows/240): fewer still)
  for (size_t k = 0; k + 1 < rb.size(); ++k) {
    CHECK(rb[k] < rb[k + 1], "slabs %llu %llu: slab %zu empty", a, b, k);
    if (k + 2 < rb.size()) CHECK(rb[k + 1] - rb[k] == slab, "slabs %llu %llu: slab %zu not of the slab size", a, b, k);
  }
}

static void check_pack(const std::vector<PackRange>& r, bool seen[16][5]) {
  static const uint64_t kLen[5] = {1, 15, 16, 17, 4096};
  std::vector<uint64_t> at;
  const uint64_t pk = pack_ranges(r, &at);
  CHECK(at.size() == r.size(), "%zu ranges", r.size());
  uint64_t end = 0;  // of the ranges placed so far
  for (size_t i = 0; i < r.size() && i < at.size(); ++i) {
    CHECK((at[i] & 15) == (r[i].dev_off & 15), "range %zu of %zu: residue", i, r.size());
    CHECK(at[i] >= end, "range %zu of %zu: overlaps the one before", i, r.size());
    end = at[i] + r[i].len;
    for (int l = 0; l < 5; ++l)
      if (r[i].len == kLen[l]) seen[r[i].dev_off & 15][l] = true;
  }
  CHECK(pk == end, "%zu ranges: packed size", r.size());
  CHECK(pk <= slot_estimate(r), "%zu ranges: %llu packed bytes above the estimate %llu", r.size(), (unsigned long long)pk,
        (unsigned long long)slot_estimate(r));
  CHECK(slot_estimate(r) % 256 == 0, "%zu ranges: estimate granule", r.size());
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  size_t cases = 0;
  char line[1 << 16];
  while (fgets(line, sizeof(line), f)) {
    char* q = line;
    uint64_t v[4];
    for (uint64_t& x : v) x = strtoull(q, &q, 10);
    while (*q == ' ') ++q;
    if (*q++ != ':') return 2;
    std::vector<uint64_t> want;
    for (char* e = q;; q = e) {
      const uint64_t b = strtoull(q, &e, 10);
      if (e == q) break;  // the end of the line
      want.push_back(b);
    }
    const uint64_t ntiles = v[0], rows = v[1], per = v[2], ramp = v[3];
    check_chunks(ntiles, rows, per, ramp != 0, want);
    ++cases;
  }
  fclose(f);
  CHECK(cases == 14 * 2 * 5 * 2, "%zu cases read", cases);
  // the slab schedule: four given cases, then rows x per around the 240-slab limit
  const std::vector<uint64_t> none{0}, one{0, 100}, six{0, 512, 1024, 1536, 2048, 2560, 3000};
  check_slabs(0, 512, &none);
  check_slabs(100, 1000, &one);
  check_slabs(3000, 512, &six);
  check_slabs(1000000, 128);
  const std::vector<uint64_t> big = slab_bounds(1000000, 128);
  CHECK(big.size() == 241 && big[1] == 4167 && big[239] == 239 * 4167ull && big[240] == 1000000, "slabs 1000000 128");
  cases += 4;
  for (uint64_t rows : {1ull, 2ull, 239ull, 240ull, 241ull, 1000ull, 4097ull, 57600ull, 999983ull, 1000000ull, 5000000000ull})
    for (uint64_t per : {0ull, 1ull, 7ull, 128ull, 512ull, 4096ull, 1ull << 20}) {
      check_slabs(rows, per);
      ++cases;
    }
  CHECK(bulk_depth(-1, false) == 3 && bulk_depth(-1, true) == 2 && bulk_depth(0, true) == 0 && bulk_depth(5, false) == 5,
        "depth");
  // range lists of 1 .. 24 ranges (kMaxScatterSegs): device offsets as in a 256-B aligned image
  // with every residue mod 16, lengths from {1, 15, 16, 17, 4096}, by a fixed generator
  static const uint64_t kLen[5] = {1, 15, 16, 17, 4096};
  bool seen[16][5] = {};
  uint64_t x = 88172645463325252ull;
  auto rnd = [&]() {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return x >> 11;
  };
  size_t lists = 0;
  for (size_t n = 0; n <= 24; ++n)
    for (int rep = 0; rep < 200; ++rep, ++lists) {
      std::vector<PackRange> r;
      uint64_t base = 0;
      for (size_t i = 0; i < n; ++i) {
        // rep 0 .. 79: one residue and one length throughout (the worst cases of the estimate)
        const uint64_t res = rep < 80 ? (uint64_t)(rep % 16) : rnd() % 16, len = rep < 80 ? kLen[rep / 16] : kLen[rnd() % 5];
        r.push_back({base + 256 * (rnd() % 64) + res, len});
        base += 256 * 128;
      }
      check_pack(r, seen);
    }
  for (int res = 0; res < 16; ++res)
    for (int l = 0; l < 5; ++l) CHECK(seen[res][l], "residue %d with length %llu never generated", res, (unsigned long long)kLen[l]);
  printf("cases %zu lists %zu failures %d\n", cases, lists, bad);
  return bad ? 1 : 0;
}
