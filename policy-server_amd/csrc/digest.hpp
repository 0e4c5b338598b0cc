// digest.hpp — the pure arithmetic of the violation digest (include/kwgpu.h kw_batch_digest): what a
// finding's key is (the bytes its message quotes from the request, or its argument as a number), the
// hash and the equality of (column, reason, allowed bit, key), the exact host reducer over words
// [rows][npol], the order and the capacity check of the output, and the geometry of the device
// reduction (reports.hip digest_*_kernel): the hash table's size under a byte budget, the status of
// one column range and the cut of the columns into halves. No HIP, no batch, no settings
// (tests/digest_check.cpp runs it on the host).
//
// What the digest replaces: one kw_format_response per finding. The message of a reason is a fixed
// text per (policy, reason) around the strings policy_message (service.cpp) quotes, so the findings
// that share (column, reason, allowed bit, key) share the message up to the container's name.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "packed.hpp"
#include "slots.hpp"

namespace kw {

// The string columns a key reads, numbered as kernels.hpp Str (digest.cpp checks the two agree).
enum : uint32_t { DG_NS = 0, DG_IMG = 1, DG_AA = 2, DG_CAPADD = 3, DG_LK = 5, DG_LV = 6, DG_NSTR = 7 };

enum DigestKind : uint32_t {
  DK_EMPTY,    // KW_R_PRIVILEGED: the message quotes nothing but the container's name
  DK_NS,       // the row's namespace
  DK_IMG,      // the image of container ctr_off[row] + ARG
  DK_CAP,      // the added capability capadd_off[ctr_off[row]] + ARG
  DK_AA,       // the AppArmor profile of container ctr_off[row] + ARG
  DK_LK,       // the key of label lbl_off[row] + ARG
  DK_LKV,      // that label's key and value
  DK_NUM       // the 16-bit ARG itself
};

KW_HD inline uint32_t digest_kind(uint32_t reason) {
  switch (reason) {
    case KW_R_PRIVILEGED: return DK_EMPTY;
    case KW_R_NAMESPACE: return DK_NS;
    case KW_R_REG_NOT_ALLOWED:
    case KW_R_REG_REJECTED:
    case KW_R_TAG_REJECTED:
    case KW_R_IMG_NOT_ALLOWED:
    case KW_R_IMG_REJECTED: return DK_IMG;
    case KW_R_CAP_NOT_ALLOWED: return DK_CAP;
    case KW_R_APPARMOR: return DK_AA;
    case KW_R_LABEL_DENIED: return DK_LK;
    case KW_R_LABEL_CONSTRAINT: return DK_LKV;
    default: return DK_NUM;
  }
}
// The string columns (bits of DG_*) a key of this kind reads.
KW_HD inline uint32_t digest_need(uint32_t kind) {
  switch (kind) {
    case DK_NS: return 1u << DG_NS;
    case DK_IMG: return 1u << DG_IMG;
    case DK_CAP: return 1u << DG_CAPADD;
    case DK_AA: return 1u << DG_AA;
    case DK_LK: return 1u << DG_LK;
    case DK_LKV: return (1u << DG_LK) | (1u << DG_LV);
    default: return 0u;
  }
}
KW_HD inline bool digest_finding(uint32_t w) { return KW_REASON(w) != 0u; }
// A finding whose full argument is in the pass's side data: it is listed, not grouped.
KW_HD inline bool digest_wide(uint32_t w) {
  const uint32_t r = KW_REASON(w);
  return KW_ARG(w) == KW_ARG_WIDE && ((r >= 1u && r <= 11u && r != (uint32_t)KW_R_NAMESPACE) || r == (uint32_t)KW_R_GROUP);
}
// What of a word a group shares beside its column and key: the reason and the KW_F_ALLOWED bit.
KW_HD inline uint32_t digest_class(uint32_t w) { return KW_REASON(w) | ((w & KW_F_ALLOWED) ? 0x100u : 0u); }

// The columns a key is cut from, on the host or on the device (the same rows in the same order as
// the words the caller pairs them with). off == nullptr: the column is not there.
struct DigestStr {
  const uint32_t* off;
  const uint8_t* bytes;
  uint64_t n;
};
struct DigestCols {
  uint64_t rows, nctr;  // ctr_off / lbl_off hold rows + 1 entries, capadd_off nctr + 1
  const uint32_t *ctr_off, *lbl_off, *capadd_off;
  DigestStr str[DG_NSTR];
};
struct DigestKey {
  const uint8_t *p0, *p1;
  uint32_t n0, n1;
  uint32_t num;
};

// One string of a column; an entity the column does not hold reads as "" (no product word names one).
KW_HD inline void digest_str(const DigestStr& s, uint64_t e, const uint8_t** p, uint32_t* n) {
  *p = nullptr;
  *n = 0;
  if (!s.off || e >= s.n) return;
  const uint32_t a = s.off[e], b = s.off[e + 1];
  *p = s.bytes + a;
  *n = b - a;
}

// The key of the finding `word` at `row` (a row of C).
KW_HD inline DigestKey digest_key(const DigestCols& C, uint64_t row, uint32_t word) {
  DigestKey k;
  k.p0 = k.p1 = nullptr;
  k.n0 = k.n1 = 0;
  k.num = 0;
  const uint32_t kind = digest_kind(KW_REASON(word)), arg = KW_ARG(word);
  if (kind == DK_NUM) {
    k.num = arg;
    return k;
  }
  if (kind == DK_EMPTY || row >= C.rows) return k;
  switch (kind) {
    case DK_NS: digest_str(C.str[DG_NS], row, &k.p0, &k.n0); break;
    case DK_IMG: digest_str(C.str[DG_IMG], (uint64_t)C.ctr_off[row] + arg, &k.p0, &k.n0); break;
    case DK_AA: digest_str(C.str[DG_AA], (uint64_t)C.ctr_off[row] + arg, &k.p0, &k.n0); break;
    case DK_CAP: {
      const uint64_t c = C.ctr_off[row];
      if (c <= C.nctr && C.capadd_off) digest_str(C.str[DG_CAPADD], (uint64_t)C.capadd_off[c] + arg, &k.p0, &k.n0);
      break;
    }
    case DK_LK: digest_str(C.str[DG_LK], (uint64_t)C.lbl_off[row] + arg, &k.p0, &k.n0); break;
    default:
      digest_str(C.str[DG_LK], (uint64_t)C.lbl_off[row] + arg, &k.p0, &k.n0);
      digest_str(C.str[DG_LV], (uint64_t)C.lbl_off[row] + arg, &k.p1, &k.n1);
      break;
  }
  return k;
}

// 64 bits over (column, class, key): FNV-1a with the lengths ahead of the bytes, then a finaliser so
// the low bits index a table.
KW_HD inline uint64_t digest_hash(uint32_t col, uint32_t cls, const DigestKey& k) {
  uint64_t h = 0xcbf29ce484222325ull;
  const uint64_t P = 0x100000001b3ull;
  h = (h ^ col) * P;
  h = (h ^ cls) * P;
  h = (h ^ k.n0) * P;
  h = (h ^ k.n1) * P;
  h = (h ^ k.num) * P;
  for (uint32_t i = 0; i < k.n0; ++i) h = (h ^ k.p0[i]) * P;
  for (uint32_t i = 0; i < k.n1; ++i) h = (h ^ k.p1[i]) * P;
  h ^= h >> 30;
  h *= 0xbf58476d1ce4e5b9ull;
  h ^= h >> 27;
  h *= 0x94d049bb133111ebull;
  h ^= h >> 31;
  return h;
}
// A slot's tag: the low `bits` of the hash (KW_DIGEST_HASH_BITS), never 0 (0 marks a free slot).
KW_HD inline uint64_t digest_tag(uint64_t h, uint32_t bits) {
  if (bits < 64u) h &= (1ull << bits) - 1ull;
  return h ? h : 1ull;
}
KW_HD inline bool digest_same_key(const DigestKey& a, const DigestKey& b) {
  if (a.n0 != b.n0 || a.n1 != b.n1 || a.num != b.num) return false;
  for (uint32_t i = 0; i < a.n0; ++i)
    if (a.p0[i] != b.p0[i]) return false;
  for (uint32_t i = 0; i < a.n1; ++i)
    if (a.p1[i] != b.p1[i]) return false;
  return true;
}

// ---- the exact reducer (host) ----
// A group's identity as an ordered map's key, no hashing: column, class and the key as one string
// (DK_LKV: the label key's length ahead of key and value; DK_NUM: the argument's two bytes; the
// reason fixes which, so the forms cannot meet).
using DigestId = std::tuple<uint32_t, uint32_t, std::string>;
struct DigestGroup {
  uint64_t first_row;
  uint32_t word;
  uint64_t count;
};
using DigestMap = std::map<DigestId, DigestGroup>;

inline std::string digest_key_string(uint32_t word, const DigestKey& k) {
  std::string s;
  const uint32_t kind = digest_kind(KW_REASON(word));
  if (kind == DK_NUM) {
    s.push_back((char)(k.num & 0xffu));
    s.push_back((char)(k.num >> 8));
    return s;
  }
  if (kind == DK_LKV) s.append((const char*)&k.n0, sizeof(k.n0));
  if (k.n0) s.append((const char*)k.p0, k.n0);
  if (k.n1) s.append((const char*)k.p1, k.n1);
  return s;
}

struct DigestAcc {
  DigestMap groups;
  std::vector<uint64_t> wide;  // pair indices row * npol + col
  uint64_t findings = 0;
};
// One finding of batch row `row` (a row of C) into the accumulator; any order of calls.
inline void digest_add(DigestAcc* A, const DigestCols& C, uint64_t row, uint32_t col, uint32_t npol, uint32_t word) {
  if (!digest_finding(word)) return;
  ++A->findings;
  if (digest_wide(word)) {
    A->wide.push_back(row * npol + col);
    return;
  }
  DigestId id(col, digest_class(word), digest_key_string(word, digest_key(C, row, word)));
  auto it = A->groups.find(id);
  if (it == A->groups.end()) {
    A->groups.emplace(std::move(id), DigestGroup{row, word, 1});
  } else {
    ++it->second.count;
    if (row < it->second.first_row) {
      it->second.first_row = row;
      it->second.word = word;
    }
  }
}
// The string columns the findings of words [rows][npol] read that C does not hold (bits of DG_*).
inline uint32_t digest_missing(const DigestCols& C, const uint32_t* words, uint64_t rows, uint32_t npol) {
  uint32_t need = 0, have = 0;
  for (uint64_t i = 0; i < rows * npol; ++i)
    if (digest_finding(words[i]) && !digest_wide(words[i])) need |= digest_need(digest_kind(KW_REASON(words[i])));
  for (uint32_t m = 0; m < DG_NSTR; ++m)
    if (C.str[m].off) have |= 1u << m;
  return need & ~have;
}
inline void digest_reduce(const DigestCols& C, const uint32_t* words, uint64_t rows, uint32_t npol, DigestAcc* A) {
  for (uint64_t r = 0; r < rows; ++r)
    for (uint32_t c = 0; c < npol; ++c) digest_add(A, C, r, c, npol, words[r * npol + c]);
}
inline void digest_records(const DigestAcc& A, std::vector<kw_digest_rec>* recs) {
  for (const auto& g : A.groups) recs->push_back(kw_digest_rec{std::get<0>(g.first), g.second.word, g.second.first_row, g.second.count});
}

// The output's order: (column, reason, first_row). Two groups of a column never share a first row
// (a pair has one word), so the order is total.
inline bool digest_rec_less(const kw_digest_rec& a, const kw_digest_rec& b) {
  if (a.col != b.col) return a.col < b.col;
  if (KW_REASON(a.word) != KW_REASON(b.word)) return KW_REASON(a.word) < KW_REASON(b.word);
  return a.first_row < b.first_row;
}
// The records into that order. Large results (a pass can have millions of groups) by a stable radix
// sort over the key's 16-bit digits, least significant first, skipping a digit all records share;
// small ones by comparison.
inline void digest_sort(std::vector<kw_digest_rec>* recs) {
  const size_t n = recs->size();
  if (n < 4096) {
    std::stable_sort(recs->begin(), recs->end(), digest_rec_less);
    return;
  }
  auto digit = [](const kw_digest_rec& r, int d) -> uint32_t {
    switch (d) {
      case 0: case 1: case 2: case 3: return (uint32_t)(r.first_row >> (16 * d)) & 0xffffu;
      case 4: return KW_REASON(r.word);
      case 5: return r.col & 0xffffu;
      default: return r.col >> 16;
    }
  };
  std::vector<kw_digest_rec> other(n);
  std::vector<size_t> at(65536 + 1);
  kw_digest_rec *src = recs->data(), *dst = other.data();
  for (int d = 0; d < 7; ++d) {
    std::fill(at.begin(), at.end(), 0);
    for (size_t i = 0; i < n; ++i) ++at[digit(src[i], d) + 1];
    if (at[digit(src[0], d) + 1] == n) continue;  // one value: the order stands
    for (size_t v = 0; v < 65536; ++v) at[v + 1] += at[v];
    for (size_t i = 0; i < n; ++i) dst[at[digit(src[i], d)]++] = src[i];
    std::swap(src, dst);
  }
  if (src != recs->data()) memcpy(recs->data(), src, n * sizeof(kw_digest_rec));
}

// Sorts and hands over: the exact n and nwide always; KW_E_NOSPACE when either array is too small
// (their contents are then unspecified: nothing is copied).
inline int digest_emit(std::vector<kw_digest_rec>* recs, std::vector<uint64_t>* wide, uint64_t findings, kw_digest* out) {
  if (!out) return KW_E_ARG;
  out->n = recs->size();
  out->nwide = wide->size();
  out->findings = findings;
  if ((out->n && out->cap && !out->recs) || (out->nwide && out->wide_cap && !out->wide)) return KW_E_ARG;
  if (out->n > out->cap || out->nwide > out->wide_cap) return KW_E_NOSPACE;
  digest_sort(recs);
  std::sort(wide->begin(), wide->end());
  if (out->n) memcpy(out->recs, recs->data(), out->n * sizeof(kw_digest_rec));
  if (out->nwide) memcpy(out->wide, wide->data(), out->nwide * sizeof(uint64_t));
  return KW_OK;
}

// ---- the device reduction's geometry ----
// An open-addressing table of slots in HBM, linear probing. tag: 0 free, else digest_tag of the
// groups that met there; count: their findings; rep: ~(batch_row << 32 | col) of the lowest (batch
// row, column) among them, kept by an unsigned max so that zeroed memory means "none yet".
struct DigestSlot {
  uint64_t tag, count, rep;
};
KW_HD inline uint64_t digest_rep(uint64_t batch_row, uint32_t col) { return ~((batch_row << 32) | col); }
KW_HD inline uint64_t digest_rep_row(uint64_t rep) { return ~rep >> 32; }
KW_HD inline uint32_t digest_rep_col(uint64_t rep) { return (uint32_t)(~rep & 0xffffffffull); }

constexpr uint32_t kDigestProbe = 512;        // slots a probe visits before it gives up (the range is cut)
constexpr uint32_t kDigestLeftCap = 1u << 16;  // entries of the leftover list
constexpr uint64_t kDigestMinSlots = 64;

// A finding whose slot holds another group: the host folds it in by the exact reducer.
struct DigestLeft {
  uint64_t pair;  // device row * npol + col
  uint32_t word, pad;
};
// What the kernels leave for the host beside the table (zeroed before a range).
struct DigestHead {
  uint64_t findings, nwide, nclaimed, nleft, nrec;
  uint32_t overflow;  // a probe gave up, or more groups than the load factor allows
  uint32_t missing;   // string columns (bits of DG_*) a finding needs that are not resident
};

// The slots of a table of `bytes` for a range of `pairs` (row, column) pairs: a power of two within
// the budget, no more than four per pair.
inline uint64_t digest_slots(uint64_t bytes, uint64_t pairs) {
  uint64_t n = kDigestMinSlots;
  while (n * 2 * sizeof(DigestSlot) <= bytes && n < 4 * pairs) n *= 2;
  return n;
}
// Load factor 1/2: the groups a table takes before the range is cut.
KW_HD inline uint64_t digest_max_groups(uint64_t nslots) { return nslots / 2; }

// The status of one column range after its count and verify launches: KW_OK, or KW_E_NOSPACE when
// the range must be cut (its groups, its wide findings or its leftovers did not fit).
inline int digest_range_status(const DigestHead& h, uint64_t nslots, uint64_t wide_cap, uint64_t left_cap) {
  if (h.overflow || h.nclaimed > digest_max_groups(nslots)) return KW_E_NOSPACE;
  if (h.nwide > wide_cap || h.nleft > left_cap) return KW_E_NOSPACE;
  return KW_OK;
}

// Columns [c0, c1) through run(c0, c1): a range that answers KW_E_NOSPACE is cut in halves, the
// lower first, each into the same block; a single column that does not fit ends the call with
// KW_E_NOSPACE, any other status at once. run leaves nothing behind when it answers KW_E_NOSPACE.
// *ranges counts the ranges that ran to the end.
template <class F>
int digest_ranges(uint32_t c0, uint32_t c1, F&& run, uint32_t* ranges) {
  if (c0 >= c1) return KW_OK;
  const int rc = run(c0, c1);
  if (rc == KW_OK) ++*ranges;
  if (rc != KW_E_NOSPACE) return rc;
  if (c1 - c0 <= 1u) return KW_E_NOSPACE;
  const uint32_t mid = c0 + (c1 - c0) / 2u;
  if (int lo = digest_ranges(c0, mid, run, ranges)) return lo;
  return digest_ranges(mid, c1, run, ranges);
}

// What `lane` of a wave of the count and verify kernels reads in round t of the unit that starts at
// row0 (pack_geom's w lanes a row, ipi rows a round): row row0 + t * ipi + lane / w, column
// 64 grp + lane % w, within the column range [c0, c1).
constexpr uint32_t kDigestRounds = 16;  // rounds of a unit: loads a lane keeps in flight
constexpr uint32_t kDigestWaves = 4;
struct DigestLane {
  uint64_t row;
  uint32_t col;
  bool on;
};
KW_HD inline DigestLane digest_lane(const PackGeom& p, uint64_t rows, uint32_t c0, uint32_t c1, uint32_t grp, uint64_t row0,
                                    uint32_t t, uint32_t lane) {
  DigestLane L;
  const uint32_t sub = lane / p.w;
  L.row = row0 + (uint64_t)t * p.ipi + sub;
  L.col = 64u * grp + lane % p.w;
  L.on = sub < p.ipi && L.row < rows && L.col >= c0 && L.col < c1;
  return L;
}
KW_HD inline uint64_t digest_unit_rows(const PackGeom& p) { return (uint64_t)p.ipi * kDigestRounds; }

}  // namespace kw
