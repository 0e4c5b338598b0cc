// members_check — the digest's drill-down (include/kwgpu.h kw_batch_digest_members,
// policy-server_amd/csrc/members.hpp) on the host, no GPU and no Python in the process
// (tests/test_members.py builds it with -fsanitize=address,undefined and runs it). Header only: the
// selection table's geometry; the table, the class masks and the probe over a made-up pass, walked
// the way the kernel walks it (digest_lane, the mask, members_find) with the hash at 64, 4 and 0 bits
// (all tags equal) and compared with the exact reducer; duplicate detection by another member of a
// group; a record list of one; the records that cannot name a group; the order of the output against
// a comparison sort, with segments on both sides of the radix threshold; the capacity arithmetic.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "members.hpp"

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

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { return rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17, rng_state; }

static uint32_t word(uint32_t reason, uint32_t arg, bool allowed = false) {
  return (reason << 8) | (arg << 16) | (allowed ? KW_F_ALLOWED : 0u);
}

// A string column in exact-size blocks: an access past either is the sanitizer's to catch.
struct Strings {
  std::vector<uint32_t> off{0};
  std::vector<uint8_t> bytes;
  void push(const std::string& s) {
    bytes.insert(bytes.end(), s.begin(), s.end());
    off.push_back((uint32_t)bytes.size());
  }
  DigestStr view() const { return DigestStr{off.data(), bytes.data(), off.size() - 1}; }
};

// A pass of rows x npol: every row one or two containers with images of a few values, a namespace of
// a few values, a label; words of reasons 2 (namespace), 3 (image of container ARG), 11 (label key
// and value), 12 (a number), allowed or not, some wide, many zero.
struct Pass {
  uint64_t rows;
  uint32_t npol;
  Strings ns, img, lk, lv;
  std::vector<uint32_t> ctr_off{0}, lbl_off{0}, capadd_off{0};
  std::vector<uint32_t> words;
  DigestCols C{};
  Pass(uint64_t r, uint32_t n) : rows(r), npol(n) {
    for (uint64_t i = 0; i < rows; ++i) {
      ns.push("ns" + std::to_string(rnd() % 5));
      const uint32_t nc = 1 + (uint32_t)(rnd() % 2);
      for (uint32_t c = 0; c < nc; ++c) img.push(std::string("reg.io/") + (char)('a' + rnd() % 7));
      ctr_off.push_back(ctr_off.back() + nc);
      lk.push(rnd() % 2 ? "ab" : "a");
      lv.push(rnd() % 2 ? "c" : "bc");
      lbl_off.push_back(lbl_off.back() + 1);
    }
    capadd_off.assign(ctr_off.back() + 1, 0);
    C.rows = rows;
    C.nctr = ctr_off.back();
    C.ctr_off = ctr_off.data();
    C.lbl_off = lbl_off.data();
    C.capadd_off = capadd_off.data();
    C.str[DG_NS] = ns.view();
    C.str[DG_IMG] = img.view();
    C.str[DG_LK] = lk.view();
    C.str[DG_LV] = lv.view();
    words.assign((size_t)(rows * npol), 0);
    for (uint64_t i = 0; i < rows; ++i)
      for (uint32_t c = 0; c < npol; ++c) {
        uint32_t w = 0;
        switch ((c + rnd() % 2) % 6) {
          case 0: w = word(2, 0, rnd() % 4 == 0); break;
          case 1: w = word(3, (uint32_t)(rnd() % (ctr_off[i + 1] - ctr_off[i]))); break;
          case 2: w = word(11, 0, rnd() % 3 == 0); break;
          case 3: w = word(12, (uint32_t)(rnd() % 3)); break;
          case 4: w = rnd() % 8 == 0 ? word(3, 0xffff) : 1u; break;  // a wide finding, or an accept
          default: w = word(0xa5, 0xa5a5); break;                    // a reason past 31: the mask aliases it
        }
        words[(size_t)(i * npol + c)] = w;
      }
  }
};

static void check_geometry() {
  ++cases;
  for (uint64_t g : {0ull, 1ull, 7ull, 8ull, 9ull, 64ull, 65ull, 483852ull, 1ull << 24}) {
    const uint64_t n = members_slots(g);
    CHECK(n >= kMembersMinSlots && (n & (n - 1)) == 0 && n >= 2 * g, "slots %llu for %llu groups", (unsigned long long)n, (unsigned long long)g);
    CHECK(n == kMembersMinSlots || n < 4 * g, "slots %llu: the smallest power of two", (unsigned long long)n);
  }
  CHECK(members_class_bit(digest_class(word(8, 0))) == 8 && members_class_bit(digest_class(word(8, 0, true))) == 40, "class bits");
  CHECK(members_class_bit(digest_class(word(0xa5, 0))) == 5 && members_class_bit(digest_class(word(255, 0, true))) == 63, "aliased reasons");
  CHECK(member_group(member_key(0xfffffffeu, 0xffffffffull)) == 0xfffffffeu && member_row(member_key(7, 0xfffffff0ull)) == 0xfffffff0ull, "key round trip");
  CHECK(member_key(1, 0) > member_key(0, 0xffffffffull), "the key orders by group, then row");
}

// The kernel's walk on the host: every lane of every round of every unit, the mask, the probe; the
// list in an order no caller may rely on (here: reversed), the counts per group.
static void walk(const Pass& P, const MembersTable& T, uint32_t bits, std::vector<uint64_t>* counts, std::vector<MemberEntry>* list) {
  const PackGeom p = pack_geom(P.npol);
  const uint64_t unit = digest_unit_rows(p);
  for (uint32_t grp = 0; grp < packed_groups(P.npol); ++grp)
    for (uint64_t row0 = 0; row0 < P.rows; row0 += unit)
      for (uint32_t t = 0; t < kDigestRounds; ++t)
        for (uint32_t lane = 0; lane < 64; ++lane) {
          const DigestLane L = digest_lane(p, P.rows, 0, P.npol, grp, row0, t, lane);
          if (!L.on) continue;
          const uint32_t v = P.words[(size_t)(L.row * P.npol + L.col)];
          if (!digest_finding(v) || digest_wide(v) || !((T.colmask[L.col] >> members_class_bit(digest_class(v))) & 1u)) continue;
          const uint32_t g = members_find(T.slots.data(), T.slots.size(), P.C, bits, L.row, L.col, v);
          if (g == kMembersNone) continue;
          ++(*counts)[g];
          list->push_back(MemberEntry{member_key(g, L.row), v, 0});
        }
  std::reverse(list->begin(), list->end());
}

struct Result {
  int rc;
  std::vector<uint64_t> off, rows;
  std::vector<uint32_t> words;
};
static Result emit(const std::vector<uint64_t>& counts, const std::vector<MemberEntry>& list, size_t ng, size_t cap, bool with_words = true) {
  Result R;
  R.off.assign(ng + 1, 0xdead);
  R.rows.assign(cap, 0);  // exact size
  R.words.assign(cap, 0);
  kw_members out{R.off.data(), R.rows.data(), with_words ? R.words.data() : nullptr, cap, 0};
  R.rc = members_offsets(counts.data(), ng, &out);
  if (R.rc == KW_OK && !members_order(list.data(), R.off.data(), ng, R.rows.data(), out.words, MembersSerial{})) R.rc = KW_E_ENGINE;
  R.rows.resize(std::min(cap, out.n));
  R.words.resize(std::min(cap, out.n));
  return R;
}

static void check_walk_against_reducer() {
  for (uint32_t npol : {1u, 5u, 64u, 70u})
    for (uint64_t rows : {1ull, 17ull, 400ull}) {
      Pass P(rows, npol);
      DigestAcc A;
      digest_reduce(P.C, P.words.data(), rows, npol, &A);
      std::vector<kw_digest_rec> all;
      digest_records(A, &all);
      digest_sort(&all);
      if (all.empty()) continue;
      std::vector<kw_digest_rec> third;
      for (size_t i = all.size(); i-- > 0;)
        if (i % 3 == 0) third.push_back(all[i]);
      for (const std::vector<kw_digest_rec>& sel : {all, third, std::vector<kw_digest_rec>(1, all[all.size() / 2])}) {
        std::vector<uint64_t> rc_counts;
        std::vector<MemberEntry> rc_list;
        CHECK(members_reduce(P.C, P.words.data(), rows, npol, sel.data(), sel.size(), &rc_counts, &rc_list) == KW_OK, "reduce");
        uint64_t n = 0;
        for (size_t g = 0; g < sel.size(); ++g) {
          CHECK(rc_counts[g] == sel[g].count, "group %zu: %llu members, the digest counted %llu", g, (unsigned long long)rc_counts[g],
                (unsigned long long)sel[g].count);
          n += rc_counts[g];
        }
        const Result want = emit(rc_counts, rc_list, sel.size(), (size_t)n);
        CHECK(want.rc == KW_OK, "the reducer's list orders");
        for (size_t g = 0; g < sel.size(); ++g) {
          CHECK(want.rows[(size_t)want.off[g]] == sel[g].first_row && want.words[(size_t)want.off[g]] == sel[g].word, "the first member is the record's");
          for (uint64_t i = want.off[g] + 1; i < want.off[g + 1]; ++i) CHECK(want.rows[(size_t)i] > want.rows[(size_t)i - 1], "rows ascend");
        }
        for (uint32_t bits : {64u, 4u, 0u}) {
          ++cases;
          MembersTable T;
          CHECK(members_table(P.C, sel.data(), sel.size(), rows, npol, bits, nullptr, &T) == KW_OK, "table of %zu groups, %u bits", sel.size(), bits);
          CHECK(T.slots.size() == members_slots(sel.size()) && T.colmask.size() == npol, "table geometry");
          size_t used = 0;
          std::vector<uint8_t> seen(sel.size(), 0);
          for (const MemberSlot& s : T.slots)
            if (s.tag) {
              ++used;
              CHECK(s.group < sel.size() && !seen[s.group]++, "a slot names one group, a group one slot");
              if (bits == 0) CHECK(s.tag == 1, "0 bits: every tag is 1");
            }
          CHECK(used == sel.size() && 2 * used <= T.slots.size(), "load factor at most 1/2");
          std::vector<uint64_t> counts(sel.size(), 0);
          std::vector<MemberEntry> list;
          walk(P, T, bits, &counts, &list);
          CHECK(counts == rc_counts, "the walk's counts, %u bits", bits);
          const Result got = emit(counts, list, sel.size(), (size_t)n);
          CHECK(got.rc == KW_OK && got.off == want.off && got.rows == want.rows && got.words == want.words,
                "npol %u rows %llu, %zu groups, %u bits: the walk's members are the reducer's", npol, (unsigned long long)rows, sel.size(), bits);
        }
      }
    }
}

static void check_records() {
  ++cases;
  Pass P(300, 6);
  DigestAcc A;
  digest_reduce(P.C, P.words.data(), P.rows, P.npol, &A);
  std::vector<kw_digest_rec> all;
  digest_records(A, &all);
  digest_sort(&all);
  size_t big = 0;
  for (size_t i = 0; i < all.size(); ++i)
    if (all[i].count > all[big].count) big = i;
  CHECK(all.size() > 8 && all[big].count > 4, "the made-up pass has groups");
  // another member of the largest group names the same group: a duplicate, whatever the hash keeps
  std::vector<uint64_t> counts;
  std::vector<MemberEntry> list;
  std::vector<kw_digest_rec> one(1, all[big]);
  CHECK(members_reduce(P.C, P.words.data(), P.rows, P.npol, one.data(), 1, &counts, &list) == KW_OK && list.size() == all[big].count, "one record");
  kw_digest_rec other = all[big];
  other.first_row = member_row(list.back().key);
  other.word = list.back().word;
  other.count = 0;
  CHECK(other.first_row != all[big].first_row, "the last member is another row");
  for (uint32_t bits : {64u, 4u, 0u}) {
    MembersTable T;
    std::vector<kw_digest_rec> dup = all;
    dup.push_back(other);
    CHECK(members_table(P.C, dup.data(), dup.size(), P.rows, P.npol, bits, nullptr, &T) == KW_E_ARG, "a duplicate by another member, %u bits", bits);
    dup.back() = all[0];
    CHECK(members_table(P.C, dup.data(), dup.size(), P.rows, P.npol, bits, nullptr, &T) == KW_E_ARG, "the same record twice, %u bits", bits);
    // named by its last member, a group has the same members
    std::vector<kw_digest_rec> by_last(1, other);
    CHECK(members_table(P.C, by_last.data(), 1, P.rows, P.npol, bits, nullptr, &T) == KW_OK && T.slots.size() == kMembersMinSlots, "a list of one");
    std::vector<uint64_t> c2(1, 0);
    std::vector<MemberEntry> l2;
    walk(P, T, bits, &c2, &l2);
    const Result a = emit(counts, list, 1, list.size()), b = emit(c2, l2, 1, l2.size());
    CHECK(a.rc == KW_OK && b.rc == KW_OK && a.rows == b.rows && a.words == b.words && a.off == b.off, "named by the last member, %u bits", bits);
  }
  CHECK(members_reduce(P.C, P.words.data(), P.rows, P.npol, std::vector<kw_digest_rec>{all[big], other}.data(), 2, &counts, &list) == KW_E_ARG,
        "the reducer finds the duplicate too");
  // records that cannot name a group
  auto bad = [&](kw_digest_rec r) {
    MembersTable T;
    std::vector<uint64_t> c;
    std::vector<MemberEntry> l;
    return members_table(P.C, &r, 1, P.rows, P.npol, 64, nullptr, &T) == KW_E_ARG &&
           members_reduce(P.C, P.words.data(), P.rows, P.npol, &r, 1, &c, &l) == KW_E_ARG;
  };
  kw_digest_rec r = all[1];
  r.col = P.npol;
  CHECK(bad(r), "col >= npol");
  r = all[1];
  r.first_row = P.rows;
  CHECK(bad(r), "first_row >= rows");
  r = all[1];
  r.word &= 0xffff00ffu;
  CHECK(bad(r), "not a finding");
  r = all[1];
  r.word = word(3, 0xffff);
  CHECK(bad(r), "a wide finding");
  r = all[1];
  r.word ^= 1u << 16;  // (the table cannot see it: the check launch does; the reducer reads the words)
  CHECK(members_reduce(P.C, P.words.data(), P.rows, P.npol, &r, 1, &counts, &list) == KW_E_ARG, "a word of another pass");
  // a row map moves the representatives, nothing else
  std::vector<uint64_t> b2d(P.rows);
  for (uint64_t i = 0; i < P.rows; ++i) b2d[i] = P.rows - 1 - i;
  MembersTable T0, T1;
  CHECK(members_table(P.C, all.data(), all.size(), P.rows, P.npol, 64, nullptr, &T0) == KW_OK &&
            members_table(P.C, all.data(), all.size(), P.rows, P.npol, 64, b2d.data(), &T1) == KW_OK, "tables");
  bool moved = T0.slots.size() == T1.slots.size() && T0.colmask == T1.colmask;
  for (size_t i = 0; moved && i < T0.slots.size(); ++i)
    moved = T0.slots[i].tag == T1.slots[i].tag && T0.slots[i].group == T1.slots[i].group &&
            (!T0.slots[i].tag || T1.slots[i].rep_row == P.rows - 1 - T0.slots[i].rep_row);
  CHECK(moved, "the row map");
  // the caller's arrays
  uint64_t off[2], rows[1];
  kw_members m{off, rows, nullptr, 1, 0};
  CHECK(members_out_ok(&r, 1, &m), "rows only");
  m.off = nullptr;
  CHECK(!members_out_ok(&r, 1, &m) && members_out_ok(nullptr, 0, &m), "off is required with groups, not without");
  m.off = off;
  m.rows = nullptr;
  CHECK(!members_out_ok(&r, 1, &m), "rows NULL with cap > 0");
  m.cap = 0;
  CHECK(members_out_ok(&r, 1, &m) && !members_out_ok(nullptr, 1, &m) && !members_out_ok(&r, 1, nullptr), "cap 0 needs no rows");
}

// The order against a comparison sort: segments below and above the radix threshold, constant digits,
// rows past 16 bits, empty groups, and lists that are not the offsets' list.
static void check_order_and_capacity() {
  for (int shape = 0; shape < 4; ++shape) {
    ++cases;
    const size_t ng = shape == 0 ? 1 : shape == 3 ? 3000 : 40;  // (shape 3: several buckets, several chunks of the list)
    std::vector<uint64_t> counts(ng, 0);
    std::vector<MemberEntry> list;
    for (size_t g = 0; g < ng; ++g) {
      const size_t n = shape == 0 ? 20000 : shape == 3 ? (g == 77 ? 90000 : 1 + (size_t)(rnd() % 140)) : g % 7 == 3 ? 0 : g == 5 ? 5000 : g == 6 ? 4096 : g == 7 ? 4095 : 1 + (size_t)(rnd() % 50);
      // distinct rows: a run of consecutive ones from a start, so digits repeat; shape 2 past 16 bits
      const uint64_t start = shape == 2 ? 0x00fe0000ull + rnd() % 70000 : rnd() % 100;
      for (size_t i = 0; i < n; ++i) list.push_back(MemberEntry{member_key((uint32_t)g, start + 3 * i), (uint32_t)rnd(), 0});
      counts[g] = n;
    }
    for (size_t i = list.size(); i > 1; --i) std::swap(list[i - 1], list[(size_t)(rnd() % i)]);
    std::vector<MemberEntry> want = list;
    std::sort(want.begin(), want.end(), [](const MemberEntry& a, const MemberEntry& b) { return a.key < b.key; });
    const Result got = emit(counts, list, ng, list.size());
    bool same = got.rc == KW_OK && got.rows.size() == want.size() && got.off[ng] == want.size();
    for (size_t i = 0; same && i < want.size(); ++i) same = got.rows[i] == member_row(want[i].key) && got.words[i] == want[i].word;
    for (size_t g = 0; same && g < ng; ++g) same = got.off[g + 1] - got.off[g] == counts[g];
    CHECK(same, "order, shape %d", shape);
    const Result rows_only = emit(counts, list, ng, list.size(), false);
    CHECK(rows_only.rc == KW_OK && rows_only.rows == got.rows, "rows only, shape %d", shape);
    // capacity: one too small and none at all keep n and off exact and write nothing
    for (size_t cap : {list.size() - 1, (size_t)0}) {
      const Result small = emit(counts, list, ng, cap);
      CHECK(small.rc == KW_E_NOSPACE && small.off == got.off, "cap %zu: KW_E_NOSPACE with the exact offsets", cap);
    }
    // a list that is not the one the offsets were counted from
    std::vector<MemberEntry> wrong = list;
    wrong[0].key = member_key((uint32_t)ng, 0);
    CHECK(emit(counts, wrong, ng, list.size()).rc == KW_E_ENGINE, "a group past the list");
    if (ng > 1) {
      wrong = list;
      for (MemberEntry& e : wrong)
        if (member_group(e.key) == 5) {
          e.key = member_key(6, member_row(e.key));
          break;
        }
      CHECK(emit(counts, wrong, ng, list.size()).rc == KW_E_ENGINE, "a member too many in one group");
    }
  }
  ++cases;
  std::vector<uint64_t> none;
  uint64_t off0[1] = {7};
  kw_members m{off0, nullptr, nullptr, 0, 9};
  CHECK(members_offsets(none.data(), 0, &m) == KW_OK && m.n == 0 && off0[0] == 0, "no groups: n = 0");
}

int main() {
  check_geometry();
  check_walk_against_reducer();
  check_records();
  check_order_and_capacity();
  printf("members_check: cases %d failures %d\n", cases, failures);
  return failures ? 1 : 0;
}
