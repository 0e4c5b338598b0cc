// digest_check — the violation digest (include/kwgpu.h kw_batch_digest,
// policy-server_amd/csrc/digest.hpp) on the host, no GPU and no Python in the process
// (tests/test_digest.py builds it with -fsanitize=address,undefined and runs it). Header only: the
// key of every reason over hand-made columns, what counts as a wide finding, the hash's tag, the
// exact reducer in any order of arrival, the order and the capacity arithmetic of the output, the
// table's size under a budget, the status of a range (the leftover list's overflow among them), the
// halving of the column range, and the kernels' lane geometry walked the way the kernels walk it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "digest.hpp"

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

using namespace kw;

// A string column in exact-size blocks: an access past either is the sanitizer's to catch.
struct Strings {
  std::vector<uint32_t> off{0};
  std::vector<uint8_t> bytes;
  void push(const char* s) {
    bytes.insert(bytes.end(), s, s + strlen(s));
    off.push_back((uint32_t)bytes.size());
  }
  DigestStr view() const { return DigestStr{off.data(), bytes.data(), off.size() - 1}; }
};

static uint32_t word(uint32_t reason, uint32_t arg, bool allowed = false) {
  return (reason << 8) | (arg << 16) | (allowed ? KW_F_ALLOWED : 0u);
}
static std::string str(const uint8_t* p, uint32_t n) { return std::string((const char*)p, n); }

// Three rows: row 0 has containers 0-1 and labels 0-1, row 1 container 2 and no label, row 2 none.
struct Fixture {
  Strings ns, img, aa, cap, lk, lv;
  std::vector<uint32_t> ctr_off{0, 2, 3, 3}, lbl_off{0, 2, 2, 2}, capadd_off{0, 1, 1, 3};
  DigestCols C{};
  Fixture() {
    for (const char* s : {"default", "kube-system", ""}) ns.push(s);
    for (const char* s : {"nginx", "evil.io/x:1", "nginx"}) img.push(s);
    for (const char* s : {"runtime/default", "", "localhost/evil"}) aa.push(s);
    for (const char* s : {"NET_ADMIN", "CHOWN", "NET_ADMIN"}) cap.push(s);
    for (const char* s : {"ab", "a"}) lk.push(s);
    for (const char* s : {"c", "bc"}) lv.push(s);
    C.rows = 3;
    C.nctr = 3;
    C.ctr_off = ctr_off.data();
    C.lbl_off = lbl_off.data();
    C.capadd_off = capadd_off.data();
    C.str[DG_NS] = ns.view();
    C.str[DG_IMG] = img.view();
    C.str[DG_AA] = aa.view();
    C.str[DG_CAPADD] = cap.view();
    C.str[DG_LK] = lk.view();
    C.str[DG_LV] = lv.view();
  }
};

static void check_keys() {
  ++cases;
  Fixture F;
  DigestKey k = digest_key(F.C, 0, word(KW_R_PRIVILEGED, 1));
  CHECK(k.n0 == 0 && k.n1 == 0 && k.num == 0, "privileged: the key is empty");
  k = digest_key(F.C, 1, word(KW_R_NAMESPACE, 0));
  CHECK(str(k.p0, k.n0) == "kube-system" && k.n1 == 0, "namespace: the row's ns");
  k = digest_key(F.C, 2, word(KW_R_NAMESPACE, 0));
  CHECK(k.n0 == 0, "namespace: an empty ns is an empty key");
  for (uint32_t r = KW_R_REG_NOT_ALLOWED; r <= (uint32_t)KW_R_IMG_REJECTED; ++r) {
    k = digest_key(F.C, 0, word(r, 1));
    CHECK(str(k.p0, k.n0) == "evil.io/x:1", "reason %u: the image of container ctr_off[row] + ARG", r);
    k = digest_key(F.C, 1, word(r, 0));
    CHECK(str(k.p0, k.n0) == "nginx", "reason %u: row 1's container", r);
  }
  k = digest_key(F.C, 1, word(KW_R_CAP_NOT_ALLOWED, 1));
  CHECK(str(k.p0, k.n0) == "NET_ADMIN", "capability: capadd_off[ctr_off[row]] + ARG (got %s)", str(k.p0, k.n0).c_str());
  k = digest_key(F.C, 0, word(KW_R_CAP_NOT_ALLOWED, 0));
  CHECK(str(k.p0, k.n0) == "NET_ADMIN", "capability: row 0's first");
  k = digest_key(F.C, 1, word(KW_R_APPARMOR, 0));
  CHECK(str(k.p0, k.n0) == "localhost/evil", "apparmor: the container's profile");
  k = digest_key(F.C, 0, word(KW_R_LABEL_DENIED, 1));
  CHECK(str(k.p0, k.n0) == "a" && k.n1 == 0, "denied label: its key");
  k = digest_key(F.C, 0, word(KW_R_LABEL_CONSTRAINT, 0));
  CHECK(str(k.p0, k.n0) == "ab" && str(k.p1, k.n1) == "c", "constrained label: key and value");
  const DigestKey k2 = digest_key(F.C, 0, word(KW_R_LABEL_CONSTRAINT, 1));
  CHECK(str(k2.p0, k2.n0) == "a" && str(k2.p1, k2.n1) == "bc", "constrained label 1");
  CHECK(!digest_same_key(k, k2), "(\"ab\", \"c\") and (\"a\", \"bc\") differ");
  CHECK(digest_key_string(word(KW_R_LABEL_CONSTRAINT, 0), k) != digest_key_string(word(KW_R_LABEL_CONSTRAINT, 1), k2),
        "and so do their map keys");
  CHECK(digest_hash(0, 11, k) != digest_hash(0, 11, k2), "and their hashes (the lengths go in first)");
  for (uint32_t r : {12u, 13u, 14u, 15u, 16u, 0xa5u}) {
    k = digest_key(F.C, 0, word(r, 0x1234));
    CHECK(k.n0 == 0 && k.n1 == 0 && k.num == 0x1234, "reason %u: the argument as a number", r);
    k = digest_key(F.C, 99, word(r, 7));
    CHECK(k.num == 7, "reason %u: whatever the row", r);
  }
  // an entity the column does not hold, a row outside the batch: "", never a read outside
  k = digest_key(F.C, 1, word(KW_R_APPARMOR, 50));
  CHECK(k.n0 == 0 && k.p0 == nullptr, "an index past the column reads as empty");
  k = digest_key(F.C, 2, word(KW_R_CAP_NOT_ALLOWED, 0));
  CHECK(k.n0 == 0, "row 2 has no capability: capadd_off[3] + 0 is past the column");
  k = digest_key(F.C, 3, word(KW_R_NAMESPACE, 0));
  CHECK(k.n0 == 0, "a row outside the batch");
  DigestCols part = F.C;
  part.str[DG_LV] = DigestStr{nullptr, nullptr, 0};
  k = digest_key(part, 0, word(KW_R_LABEL_CONSTRAINT, 0));
  CHECK(k.n0 == 2 && k.n1 == 0, "an absent column reads as empty");
  std::vector<uint32_t> ws{word(KW_R_LABEL_CONSTRAINT, 0), word(KW_R_PRIVILEGED, 0), 0};
  CHECK(digest_missing(part, ws.data(), 1, 3) == (1u << DG_LV), "digest_missing names the value column");
  CHECK(digest_missing(F.C, ws.data(), 1, 3) == 0, "and nothing on the whole batch");
  CHECK(digest_need(DK_LKV) == ((1u << DG_LK) | (1u << DG_LV)) && digest_need(DK_NUM) == 0 && digest_need(DK_EMPTY) == 0, "needs");
}

static void check_wide_and_tags() {
  ++cases;
  for (uint32_t r = 0; r < 256; ++r) {
    const bool want = (r >= 1 && r <= 11 && r != 2) || r == 13;
    CHECK(digest_wide(word(r, 0xffff)) == want, "reason %u with ARG 0xffff: wide %d", r, (int)want);
    CHECK(!digest_wide(word(r, 0xfffe)), "reason %u with ARG 0xfffe is never wide", r);
    CHECK(digest_finding(word(r, 0)) == (r != 0), "reason %u: a finding iff non-zero", r);
  }
  CHECK(digest_class(word(8, 3, true)) != digest_class(word(8, 3, false)), "the allowed bit is part of the class");
  CHECK(digest_class(word(8, 3)) == digest_class(word(8, 9) | KW_V_MUTATED | KW_BYPASS), "no other bit is");
  CHECK(digest_tag(0, 64) == 1 && digest_tag(0x1234, 0) == 1 && digest_tag(~0ull, 64) == ~0ull, "a tag is never 0");
  for (uint64_t h : {0ull, 1ull, 0xfedcba9876543210ull, ~0ull}) {
    CHECK(digest_tag(h, 4) >= 1 && digest_tag(h, 4) <= 15, "four bits: 1..15");
    CHECK(digest_tag(h, 63) <= 0x7fffffffffffffffull, "63 bits");
  }
  CHECK(digest_rep_row(digest_rep(0xfffffffeull, 0xabcdu)) == 0xfffffffeull && digest_rep_col(digest_rep(5, 0xabcdu)) == 0xabcdu, "rep round trip");
  CHECK(digest_rep(3, 9) > digest_rep(4, 0) && digest_rep(3, 1) > digest_rep(3, 2) && digest_rep(0, 0) > 0, "the max keeps the lowest (row, col)");
}

// The reducer: hand-made words over the fixture, in row-major order and in reverse.
static void check_reduce_and_emit() {
  ++cases;
  Fixture F;
  const uint32_t npol = 4;
  // col 0: capabilities; col 1: images; col 2: a wide cause mask, a number; col 3: label constraints, allowed or not
  std::vector<uint32_t> w{
      word(8, 0), word(3, 1),      word(13, 0xffff), word(11, 0),
      word(8, 1), word(3, 0),      word(12, 2),      word(11, 0, true),
      0,          word(3, 0xffff), word(12, 2),      1u};
  DigestAcc A, B;
  digest_reduce(F.C, w.data(), 3, npol, &A);
  for (uint64_t i = w.size(); i-- > 0;) digest_add(&B, F.C, i / npol, (uint32_t)(i % npol), npol, w[i]);
  std::vector<kw_digest_rec> ra, rb;
  digest_records(A, &ra);
  digest_records(B, &rb);
  kw_digest_rec got[8];
  uint64_t wide[4];
  kw_digest out{got, 8, 0, wide, 4, 0, 0};
  CHECK(digest_emit(&ra, &A.wide, A.findings, &out) == KW_OK, "emit");
  CHECK(out.findings == 10 && out.nwide == 2 && wide[0] == 2 && wide[1] == 9, "findings %llu wide %zu", (unsigned long long)out.findings, out.nwide);
  // groups: col 0 NET_ADMIN x2 (rows 0, 1: row 1's arg 1 is capadd_off[2] + 1); col 1 evil.io/x:1 (row 0), nginx (row 1);
  // col 2 number 2 x2 (rows 1, 2); col 3 ("ab", "c") rejected (row 0); col 3 row 1 has no label: "" allowed
  const kw_digest_rec want[6] = {{0, word(8, 0), 0, 2}, {1, word(3, 1), 0, 1}, {1, word(3, 0), 1, 1},
                                 {2, word(12, 2), 1, 2}, {3, word(11, 0), 0, 1}, {3, word(11, 0, true), 1, 1}};
  CHECK(out.n == 6, "groups %zu", out.n);
  for (size_t i = 0; i < 6 && i < out.n; ++i)
    CHECK(got[i].col == want[i].col && got[i].word == want[i].word && got[i].first_row == want[i].first_row && got[i].count == want[i].count,
          "record %zu: col %u word %#x first %llu count %llu", i, got[i].col, got[i].word, (unsigned long long)got[i].first_row,
          (unsigned long long)got[i].count);
  kw_digest_rec got2[8];
  uint64_t wide2[4];
  kw_digest out2{got2, 8, 0, wide2, 4, 0, 0};
  CHECK(digest_emit(&rb, &B.wide, B.findings, &out2) == KW_OK && out2.n == out.n && !memcmp(got, got2, out.n * sizeof(got[0])) &&
            out2.nwide == 2 && wide2[0] == 2 && wide2[1] == 9,
        "the order of arrival does not change the records or the wide list");
  uint64_t sum = 0;
  for (size_t i = 0; i < out.n; ++i) sum += got[i].count;
  CHECK(sum + out.nwide == out.findings, "counts + wide = findings");
  // the capacity arithmetic: one too small either way, the exact needs, nothing written past the caps
  {
    std::vector<kw_digest_rec> small(5);
    std::vector<uint64_t> sw(2);
    kw_digest o{small.data(), 5, 99, sw.data(), 2, 99, 0};
    CHECK(digest_emit(&ra, &A.wide, A.findings, &o) == KW_E_NOSPACE && o.n == 6 && o.nwide == 2 && o.findings == 10, "recs one too small");
    std::vector<kw_digest_rec> fit(6);
    std::vector<uint64_t> sw1(1);
    kw_digest o2{fit.data(), 6, 0, sw1.data(), 1, 0, 0};
    CHECK(digest_emit(&ra, &A.wide, A.findings, &o2) == KW_E_NOSPACE && o2.n == 6 && o2.nwide == 2, "wide one too small");
    kw_digest o3{nullptr, 0, 0, nullptr, 0, 0, 0};
    CHECK(digest_emit(&ra, &A.wide, A.findings, &o3) == KW_E_NOSPACE && o3.n == 6 && o3.nwide == 2, "no arrays: the needs");
    kw_digest o4{fit.data(), 6, 0, sw.data(), 2, 0, 0};
    CHECK(digest_emit(&ra, &A.wide, A.findings, &o4) == KW_OK, "exactly enough");
    std::vector<kw_digest_rec> none;
    std::vector<uint64_t> nw;
    CHECK(digest_emit(&none, &nw, 0, &o3) == KW_OK && o3.n == 0 && o3.nwide == 0 && o3.findings == 0, "an empty digest needs no arrays");
    CHECK(digest_emit(&none, &nw, 0, nullptr) == KW_E_ARG, "no output struct");
  }
  // the order is (col, reason, first_row)
  CHECK(digest_rec_less({0, word(9, 0), 5, 1}, {1, word(3, 0), 0, 1}) && digest_rec_less({1, word(3, 0), 9, 1}, {1, word(4, 0), 0, 1}) &&
            digest_rec_less({1, word(3, 7), 2, 1}, {1, word(3, 0), 3, 1}) && !digest_rec_less({1, word(3, 0), 3, 1}, {1, word(3, 7), 3, 1}),
        "record order");
}

static void check_table_and_status() {
  ++cases;
  for (uint64_t bytes : {1ull, 24ull, 1535ull, 1536ull, 3072ull, 100000ull, 64ull << 20, 1ull << 40})
    for (uint64_t pairs : {1ull, 16ull, 17ull, 1000ull, 64000000ull}) {
      const uint64_t n = digest_slots(bytes, pairs);
      CHECK(n >= kDigestMinSlots && (n & (n - 1)) == 0, "slots %llu: a power of two, at least the minimum", (unsigned long long)n);
      CHECK(n == kDigestMinSlots || n * sizeof(DigestSlot) <= bytes, "slots %llu within %llu bytes", (unsigned long long)n, (unsigned long long)bytes);
      CHECK(n == kDigestMinSlots || n < 8 * pairs, "slots %llu: no more than the pairs call for (%llu)", (unsigned long long)n, (unsigned long long)pairs);
      CHECK(n * 2 * sizeof(DigestSlot) > bytes || n >= 4 * pairs, "slots %llu: the largest that fits", (unsigned long long)n);
    }
  CHECK(digest_slots(64ull << 20, 64000000ull) == (2ull << 20), "64 MB: 2 M slots of 24 bytes");
  DigestHead h{};
  CHECK(digest_range_status(h, 64, 10, 10) == KW_OK, "an empty range");
  h.nclaimed = 32;
  CHECK(digest_range_status(h, 64, 10, 10) == KW_OK, "half the slots");
  h.nclaimed = 33;
  CHECK(digest_range_status(h, 64, 10, 10) == KW_E_NOSPACE, "more than half the slots");
  h.nclaimed = 1;
  h.overflow = 1;
  CHECK(digest_range_status(h, 64, 10, 10) == KW_E_NOSPACE, "a probe gave up");
  h.overflow = 0;
  h.nwide = 11;
  CHECK(digest_range_status(h, 64, 10, 10) == KW_E_NOSPACE, "the wide list overflowed");
  h.nwide = 10;
  h.nleft = kDigestLeftCap;
  CHECK(digest_range_status(h, 64, 10, kDigestLeftCap) == KW_OK, "the leftover list exactly full");
  h.nleft = kDigestLeftCap + 1ull;
  CHECK(digest_range_status(h, 64, 10, kDigestLeftCap) == KW_E_NOSPACE, "the leftover list overflowed: the range is cut");
}

// The halving over a made-up pass: column c has groups[c] groups, a range fits while its sum <= room.
static void check_ranges() {
  ++cases;
  struct Case {
    std::vector<uint32_t> groups;
    uint32_t room;
    int want;
  };
  std::vector<uint32_t> many(128, 10);
  many[77] = 300;
  const Case cs[] = {{{1, 2, 3}, 6, KW_OK}, {{1, 2, 3}, 5, KW_OK}, {{5, 5, 5, 5, 5}, 5, KW_OK}, {{5, 6, 5}, 5, KW_E_NOSPACE},
                     {{7}, 6, KW_E_NOSPACE}, {{}, 1, KW_OK}, {many, 320, KW_OK}, {many, 299, KW_E_NOSPACE}, {std::vector<uint32_t>(128, 3), 100, KW_OK}};
  for (const Case& c : cs) {
    std::vector<uint32_t> seen(c.groups.size(), 0);
    uint32_t last_end = 0, calls = 0, done = 0;
    bool ordered = true;
    auto run = [&](uint32_t c0, uint32_t c1) -> int {
      ++calls;
      uint64_t sum = 0;
      for (uint32_t k = c0; k < c1; ++k) sum += c.groups[k];
      if (sum > c.room) return KW_E_NOSPACE;
      if (c0 != last_end) ordered = false;
      last_end = c1;
      for (uint32_t k = c0; k < c1; ++k) ++seen[k];
      return KW_OK;
    };
    const int rc = digest_ranges(0, (uint32_t)c.groups.size(), run, &done);
    CHECK(rc == c.want, "ranges over %zu columns with room %u: %d, want %d", c.groups.size(), c.room, rc, c.want);
    CHECK(ordered, "ranges run in column order");
    if (rc == KW_OK) {
      for (size_t k = 0; k < seen.size(); ++k) CHECK(seen[k] == 1, "column %zu reduced %u times", k, seen[k]);
      CHECK(last_end == c.groups.size(), "the ranges end at the last column");
    }
    CHECK(done <= calls && calls <= 2 * c.groups.size() + 1, "%u calls for %zu columns", calls, c.groups.size());
  }
  // 128 columns of 3 groups with room for 100: 32 columns a range fit (96), so at least three ranges
  {
    uint32_t done = 0;
    auto run = [&](uint32_t c0, uint32_t c1) -> int { return (c1 - c0) * 3 > 100 ? KW_E_NOSPACE : KW_OK; };
    CHECK(digest_ranges(0, 128, run, &done) == KW_OK && done == 4, "four ranges of 32 columns (%u)", done);
  }
  // any other status ends the call at once
  {
    uint32_t done = 0, calls = 0;
    auto run = [&](uint32_t c0, uint32_t c1) -> int { return ++calls, c1 - c0 > 1 ? KW_E_NOSPACE : c0 >= 2 ? KW_E_DEVICE : KW_OK; };
    CHECK(digest_ranges(0, 4, run, &done) == KW_E_DEVICE && done == 2 && calls == 6, "a device error ends the call (%u calls)", calls);
  }
}

// The radix sort against the comparison sort, over records with many equal digits and with rows and
// columns past 16 and 32 bits.
static void check_sort() {
  uint64_t x = 88172645463325252ull;
  auto rnd = [&]() { return x ^= x << 13, x ^= x >> 7, x ^= x << 17, x; };
  for (size_t n : {0u, 1u, 4095u, 4096u, 20000u})
    for (int shape = 0; shape < 3; ++shape) {
      ++cases;
      std::vector<kw_digest_rec> a(n);
      for (size_t i = 0; i < n; ++i) {
        a[i].col = shape == 0 ? 0u : shape == 1 ? (uint32_t)(rnd() % 64) : (uint32_t)rnd();
        a[i].word = word((uint32_t)(rnd() % (shape == 0 ? 2 : 256)), (uint32_t)(rnd() & 0xffff));
        a[i].first_row = shape == 2 ? rnd() : rnd() % (shape == 0 ? 1000000u : 300u);
        a[i].count = i;  // tells equal keys apart: the sort is stable
      }
      std::vector<kw_digest_rec> want = a;
      std::stable_sort(want.begin(), want.end(), digest_rec_less);
      digest_sort(&a);
      CHECK(a.size() == want.size() && (n == 0 || !memcmp(a.data(), want.data(), n * sizeof(a[0]))), "sort of %zu records, shape %d", n, shape);
    }
}

// The kernels' walk: every (row, column of the range) exactly once, nothing outside.
static void check_lanes() {
  for (uint32_t npol : {1u, 2u, 31u, 32u, 33u, 63u, 64u, 65u, 128u, 200u})
    for (uint64_t rows : {1ull, 15ull, 16ull, 17ull, 63ull, 64ull, 65ull, 1000ull}) {
      const uint32_t ranges[][2] = {{0, npol}, {npol / 2, npol}, {0, (npol + 1) / 2}, {npol - 1, npol}};
      for (const auto& cr : ranges) {
        const uint32_t c0 = cr[0], c1 = cr[1];
        if (c0 >= c1) continue;
        ++cases;
        const PackGeom p = pack_geom(npol);
        const uint64_t unit = digest_unit_rows(p);
        std::vector<uint8_t> seen((size_t)(rows * npol), 0);  // exact size
        size_t bad = 0;
        for (uint32_t grp = c0 / 64u; grp <= (c1 - 1u) / 64u; ++grp)
          for (uint64_t row0 = 0; row0 < rows; row0 += unit)
            for (uint32_t t = 0; t < kDigestRounds; ++t)
              for (uint32_t lane = 0; lane < 64; ++lane) {
                const DigestLane L = digest_lane(p, rows, c0, c1, grp, row0, t, lane);
                if (!L.on) continue;
                if (L.row >= rows || L.col < c0 || L.col >= c1 || L.row < row0 || L.row >= row0 + unit) {
                  ++bad;
                  continue;
                }
                if (seen[(size_t)(L.row * npol + L.col)]++) ++bad;
              }
        for (uint64_t r = 0; r < rows; ++r)
          for (uint32_t c = 0; c < npol; ++c)
            if (seen[(size_t)(r * npol + c)] != (c >= c0 && c < c1 ? 1 : 0)) ++bad;
        CHECK(bad == 0, "npol %u rows %llu range [%u, %u): %zu pairs missed, repeated or outside", npol, (unsigned long long)rows, c0, c1, bad);
      }
    }
}

int main() {
  check_keys();
  check_wide_and_tags();
  check_reduce_and_emit();
  check_table_and_status();
  check_ranges();
  check_sort();
  check_lanes();
  printf("digest_check: cases %d failures %d\n", cases, failures);
  return failures ? 1 : 0;
}
