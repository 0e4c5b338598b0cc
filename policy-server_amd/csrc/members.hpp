// members.hpp — the pure arithmetic of the digest's drill-down (include/kwgpu.h
// kw_batch_digest_members): which findings of a pass are the members of the groups a caller names by
// their digest records. The validation of a record list, the exact host reducer over words
// [rows][npol] (an ordered map over DigestId, no hashing), the selection table the device walk probes
// (reports.hip members_*_kernel) with its geometry and its per-column class masks, the probe itself
// (host and device run the same function), and the order and the capacity check of the output. The
// key, the hash, the tag and the class are digest.hpp's, unchanged. No HIP, no batch, no settings
// (tests/members_check.cpp runs it on the host).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "digest.hpp"

namespace kw {

constexpr uint32_t kMembersNone = 0xffffffffu;  // no group

// One member as the walk appends it and the host orders it: key = group << 32 | batch row (both
// < 2^32), so the output's order (group, row) is the order of the keys.
struct MemberEntry {
  uint64_t key;
  uint32_t word, pad;
};
KW_HD inline uint64_t member_key(uint32_t group, uint64_t batch_row) { return ((uint64_t)group << 32) | batch_row; }
KW_HD inline uint32_t member_group(uint64_t key) { return (uint32_t)(key >> 32); }
KW_HD inline uint64_t member_row(uint64_t key) { return key & 0xffffffffull; }

// A slot of the selection table: open addressing, linear probing, one named group a slot (groups
// whose tags are equal lie in different slots, so a probe compares keys until a free slot ends it).
// tag: 0 free, else digest_tag of the group; rep_row: the representative's row in the rows the
// walk's columns speak (device rows on the device), word its verdict word, col its column.
struct MemberSlot {
  uint64_t tag, rep_row;
  uint32_t group, col, word, pad;
};
// What the kernels leave for the host beside the per-group counts (zeroed before the launches).
struct MembersHead {
  uint64_t nlist;  // members found: the list holds the first min(nlist, its capacity)
  uint32_t bad;    // a representative's word is not the pass's word at its pair
  uint32_t pad;
};

// The slots for ngroups named groups: a power of two, load factor at most 1/2 (so a probe always
// meets a free slot).
constexpr uint64_t kMembersMinSlots = 16;
inline uint64_t members_slots(uint64_t ngroups) {
  uint64_t n = kMembersMinSlots;
  while (n < 2 * ngroups) n *= 2;
  return n;
}

// The bit of a class in a column's 64-bit mask of selected classes: the reason's low five bits and
// the allowed bit. Reasons of 32 and more share bits with lower ones; the mask only spares a finding
// the read of its key bytes, the probe decides.
KW_HD inline uint32_t members_class_bit(uint32_t cls) { return (cls & 31u) | ((cls & 0x100u) ? 32u : 0u); }

// A record that can name a group of a pass of rows x npol: a finding that is not wide, inside the pass.
inline bool members_rec_ok(const kw_digest_rec& r, uint64_t rows, uint32_t npol) {
  return r.col < npol && r.first_row < rows && digest_finding(r.word) && !digest_wide(r.word);
}
// The caller's arrays (the rules of the header).
inline bool members_out_ok(const kw_digest_rec* groups, size_t ngroups, const kw_members* out) {
  if (!out || (ngroups && (!groups || !out->off)) || (out->cap && !out->rows)) return false;
  return ngroups < kMembersNone;
}

// The named group the finding `word` at (row, col) belongs to, or kMembersNone: the probe from its
// tag's slot on, comparing column, class and key bytes with each equal-tagged slot's representative
// (as digest_verify_kernel compares), to the first free slot. Exact whatever the hash does. `row`
// and the slots' rep_row are rows of C.
KW_HD inline uint32_t members_find(const MemberSlot* table, uint64_t nslots, const DigestCols& C, uint32_t hash_bits,
                                   uint64_t row, uint32_t col, uint32_t word) {
  const DigestKey key = digest_key(C, row, word);
  const uint32_t cls = digest_class(word);
  const uint64_t tag = digest_tag(digest_hash(col, cls, key), hash_bits), mask = nslots - 1u;
  uint64_t i = tag & mask;
  for (uint64_t probe = 0; probe < nslots; ++probe, i = (i + 1u) & mask) {
    const MemberSlot s = table[i];
    if (s.tag == 0u) return kMembersNone;
    if (s.tag == tag && s.col == col && digest_class(s.word) == cls && digest_same_key(key, digest_key(C, s.rep_row, s.word)))
      return s.group;
  }
  return kMembersNone;
}

// The selection table over the records and each column's class mask. H: the host columns (batch
// rows); b2d: the row of each batch row in the rows the walk reads (nullptr: the same). KW_E_ARG for
// a record that cannot name a group and for two records of one group (equal column, class and key
// bytes: found among the slots of equal tags on the way to the record's own).
struct MembersTable {
  std::vector<MemberSlot> slots;
  std::vector<uint64_t> colmask;  // [npol]
};
inline int members_table(const DigestCols& H, const kw_digest_rec* groups, size_t ngroups, uint64_t rows, uint32_t npol,
                         uint32_t hash_bits, const uint64_t* b2d, MembersTable* T) {
  if (ngroups >= kMembersNone) return KW_E_ARG;
  T->slots.assign((size_t)members_slots(ngroups), MemberSlot{0, 0, 0, 0, 0, 0});
  T->colmask.assign(npol, 0);
  const uint64_t mask = T->slots.size() - 1u;
  for (size_t g = 0; g < ngroups; ++g) {
    const kw_digest_rec& r = groups[g];
    if (!members_rec_ok(r, rows, npol)) return KW_E_ARG;
    const DigestKey key = digest_key(H, r.first_row, r.word);
    const uint32_t cls = digest_class(r.word);
    const uint64_t tag = digest_tag(digest_hash(r.col, cls, key), hash_bits);
    uint64_t i = tag & mask;
    for (;; i = (i + 1u) & mask) {  // (load factor 1/2: a free slot is there)
      const MemberSlot& s = T->slots[(size_t)i];
      if (s.tag == 0u) break;
      if (s.tag == tag && s.col == r.col && digest_class(s.word) == cls &&
          digest_same_key(key, digest_key(H, groups[s.group].first_row, s.word)))
        return KW_E_ARG;
    }
    T->slots[(size_t)i] = MemberSlot{tag, b2d ? b2d[r.first_row] : r.first_row, (uint32_t)g, r.col, r.word, 0};
    T->colmask[r.col] |= 1ull << members_class_bit(cls);
  }
  return KW_OK;
}

// The string columns (bits of DG_*) the records' keys read.
inline uint32_t members_need(const kw_digest_rec* groups, size_t ngroups) {
  uint32_t need = 0;
  for (size_t g = 0; g < ngroups; ++g) need |= digest_need(digest_kind(KW_REASON(groups[g].word)));
  return need;
}

// ---- the exact reducer (host) ----
// The members of the named groups from full words [rows][npol] in the rows of C: per-group counts
// and the list in (row, column) order of the walk, so each group's entries ascend already. KW_E_ARG
// for a bad record, a record whose word is not the pass's word at its pair, and two records of one
// group.
inline int members_reduce(const DigestCols& C, const uint32_t* words, uint64_t rows, uint32_t npol, const kw_digest_rec* groups,
                          size_t ngroups, std::vector<uint64_t>* counts, std::vector<MemberEntry>* list) {
  if (ngroups >= kMembersNone) return KW_E_ARG;
  std::map<DigestId, uint32_t> named;
  std::vector<uint64_t> colmask(npol, 0);
  for (size_t g = 0; g < ngroups; ++g) {
    const kw_digest_rec& r = groups[g];
    if (!members_rec_ok(r, rows, npol) || words[r.first_row * npol + r.col] != r.word) return KW_E_ARG;
    DigestId id(r.col, digest_class(r.word), digest_key_string(r.word, digest_key(C, r.first_row, r.word)));
    if (!named.emplace(std::move(id), (uint32_t)g).second) return KW_E_ARG;
    colmask[r.col] |= 1ull << members_class_bit(digest_class(r.word));
  }
  counts->assign(ngroups, 0);
  list->clear();
  if (ngroups == 0) return KW_OK;
  for (uint64_t r = 0; r < rows; ++r)
    for (uint32_t c = 0; c < npol; ++c) {
      const uint32_t w = words[r * npol + c];
      if (!digest_finding(w) || digest_wide(w) || !((colmask[c] >> members_class_bit(digest_class(w))) & 1u)) continue;
      const auto it = named.find(DigestId(c, digest_class(w), digest_key_string(w, digest_key(C, r, w))));
      if (it == named.end()) continue;
      ++(*counts)[it->second];
      list->push_back(MemberEntry{member_key(it->second, r), w, 0});
    }
  return KW_OK;
}

// ---- the output ----
// off and n from the exact counts, always; KW_E_NOSPACE when the members do not fit (rows and words
// are then left alone).
inline int members_offsets(const uint64_t* counts, size_t ngroups, kw_members* out) {
  uint64_t at = 0;
  for (size_t g = 0; g < ngroups; ++g) {
    out->off[g] = at;
    at += counts[g];
  }
  if (out->off) out->off[ngroups] = at;
  out->n = (size_t)at;
  return at > out->cap ? KW_E_NOSPACE : KW_OK;
}

// A stable counting pass over one 16-bit digit of the rows of src[0, n) into dst; false (nothing
// moved) when all entries share the digit. at: 65537 counters.
inline bool members_row_pass(const MemberEntry* src, MemberEntry* dst, size_t n, int d, std::vector<size_t>* at) {
  auto digit = [d](const MemberEntry& e) -> uint32_t { return (uint32_t)(e.key >> (16 * d)) & 0xffffu; };
  std::fill(at->begin(), at->end(), 0);
  for (size_t i = 0; i < n; ++i) ++(*at)[digit(src[i]) + 1];
  if ((*at)[digit(src[0]) + 1] == n) return false;  // one value: the order stands
  for (size_t v = 0; v < 65536; ++v) (*at)[v + 1] += (*at)[v];
  for (size_t i = 0; i < n; ++i) dst[(*at)[digit(src[i])]++] = src[i];
  return true;
}

constexpr size_t kMembersTask = 1u << 16;  // entries of one ordering task, about
constexpr size_t kMembersChunks = 64;      // parts of the list the first two passes run over, at most

// The n = off[ngroups] entries of `list` (any order) into rows and words (words may be null) by
// (group, row), in counting passes spread through run(ntasks, fn) (the host workers' parallel-for,
// or a loop). The groups are cut into buckets of whole groups of about kMembersTask entries, whose
// places off gives. The list, in chunks: each chunk counts its entries per bucket, then moves them to
// its share of each bucket. The buckets, each on its own: a stable radix sort over the rows' two
// 16-bit digits, skipping a digit all entries share (as digest_sort does), then one stable move of
// the entries to their groups' ranges, and out. A short list is sorted by comparison. An entry whose
// group is not < ngroups, or more entries of a group than its range: false, the list is not the one
// the offsets were counted from.
template <class Run>
bool members_order(const MemberEntry* list, const uint64_t* off, size_t ngroups, uint64_t* rows, uint32_t* words, Run&& run) {
  const size_t n = (size_t)off[ngroups];
  if (n == 0) return true;
  std::unique_ptr<MemberEntry[]> one(new MemberEntry[n]);  // (not zeroed: every entry is written before it is read)
  if (n < 4096) {
    std::copy(list, list + n, one.get());
    std::sort(one.get(), one.get() + n, [](const MemberEntry& a, const MemberEntry& b) { return a.key < b.key; });
    for (size_t g = 0, i = 0; g < ngroups; ++g)
      for (; i < (size_t)off[g + 1]; ++i)
        if (member_group(one[i].key) != g) return false;
    for (size_t i = 0; i < n; ++i) {
      rows[i] = member_row(one[i].key);
      if (words) words[i] = one[i].word;
    }
    return true;
  }
  std::unique_ptr<MemberEntry[]> two(new MemberEntry[n]);
  std::vector<size_t> cut{0};  // buckets of whole groups
  std::vector<uint32_t> bucket_of(ngroups);
  for (size_t g = 0, g0 = 0; g < ngroups; ++g) {
    bucket_of[g] = (uint32_t)(cut.size() - 1);
    if (off[g + 1] - off[g0] >= kMembersTask || g + 1 == ngroups) {
      cut.push_back(g + 1);
      g0 = g + 1;
    }
  }
  const size_t nb = cut.size() - 1, nc = std::min(kMembersChunks, (n + kMembersTask - 1) / kMembersTask);
  std::vector<uint64_t> at(nc * nb, 0);  // [chunk][bucket]: the count, then the chunk's place in the bucket
  std::atomic<bool> bad{false};
  run(nc, [&](size_t c) {
    uint64_t* h = at.data() + c * nb;
    for (size_t i = c * n / nc, e = (c + 1) * n / nc; i < e; ++i) {
      const uint32_t g = member_group(list[i].key);
      if (g >= ngroups) {
        bad = true;
        return;
      }
      ++h[bucket_of[g]];
    }
  });
  if (bad) return false;
  for (size_t b = 0; b < nb; ++b) {
    uint64_t place = off[cut[b]];
    for (size_t c = 0; c < nc; ++c) {
      const uint64_t k = at[c * nb + b];
      at[c * nb + b] = place;
      place += k;
    }
    if (place != off[cut[b + 1]]) return false;
  }
  run(nc, [&](size_t c) {
    uint64_t* h = at.data() + c * nb;
    for (size_t i = c * n / nc, e = (c + 1) * n / nc; i < e; ++i) one[(size_t)h[bucket_of[member_group(list[i].key)]]++] = list[i];
  });
  run(nb, [&](size_t b) {
    const size_t g0 = cut[b], g1 = cut[b + 1], a = (size_t)off[g0], m = (size_t)(off[g1] - off[g0]);
    if (m == 0) return;
    MemberEntry *src = one.get() + a, *dst = two.get() + a;
    std::vector<size_t> counters(65536 + 1);
    for (int d = 0; d < 2; ++d)
      if (members_row_pass(src, dst, m, d, &counters)) std::swap(src, dst);
    if (g1 - g0 > 1) {  // the rows ascend: a stable move to the groups' ranges keeps them so
      std::vector<uint64_t> cur(off + g0, off + g1);
      for (size_t i = 0; i < m; ++i) {
        const size_t g = member_group(src[i].key) - g0;
        if (cur[g] >= off[g0 + g + 1]) {
          bad = true;
          return;
        }
        dst[(size_t)(cur[g]++ - a)] = src[i];
      }
      std::swap(src, dst);
    }
    for (size_t i = 0; i < m; ++i) {
      rows[a + i] = member_row(src[i].key);
      if (words) words[a + i] = src[i].word;
    }
  });
  return !bad;
}
// (the loop that stands in for the host workers)
struct MembersSerial {
  template <class F>
  void operator()(size_t n, F&& fn) const {
    for (size_t i = 0; i < n; ++i) fn(i);
  }
};

}  // namespace kw
