// packed.hpp — the pure arithmetic of the packed verdict form (include/kwgpu.h kw_packed): a 2-bit
// code per (row, column) in two bit-planes per 64-column group, a dictionary of three words per
// column, and the words the dictionary does not hold ("exceptions") in row-major order behind a
// per-row offset. The dictionary, the array sizes, the reference host encoder, word(row, col) and
// the expansion of a row range; the device pack kernels (reports.hip) share the code function, the
// item numbering and the wave geometry. No HIP, no batch, no settings (tests/packed_check.cpp runs
// it on the host).
#pragma once
#include <cstddef>
#include <cstdint>

#include "slots.hpp"

namespace kw {

// Column groups of 64, and the u64 plane words / items of a pass. An item is one (row, group):
// item = row * G + g, its planes at planes[2 * item] (low bits) and planes[2 * item + 1] (high bits).
KW_HD inline uint32_t packed_groups(uint32_t npol) { return (npol + 63u) / 64u; }
KW_HD inline uint64_t packed_items(uint64_t rows, uint32_t npol) { return rows * packed_groups(npol); }
KW_HD inline uint64_t packed_plane_words(uint64_t rows, uint32_t npol) { return 2 * packed_items(rows, npol); }
// A pass the u32 offsets cannot index (kw_validate_host_packed: KW_E_ARG).
KW_HD inline bool packed_fits(uint64_t rows, uint32_t npol) {
  return npol != 0 && rows <= 0xffffffffull / npol;  // rows x npol < 2^32
}

constexpr uint32_t kPackEscape = 3;  // the code of a word the column's dictionary does not hold
// The code of word w under its column's dictionary d[0..3): the lowest matching index, else escape.
KW_HD inline uint32_t packed_code(uint32_t w, uint32_t d0, uint32_t d1, uint32_t d2) {
  return w == d0 ? 0u : w == d1 ? 1u : w == d2 ? 2u : kPackEscape;
}

// A column's dictionary: the word of an accepted response, of an accepted and mutated one, and of a
// bypassed request (slots.hpp finish_word, kBypassWord). Groups: a2m = 0, as slotplan.cpp.
inline void packed_dict_entry(uint32_t mode, uint32_t a2m, int origin, uint32_t d[3]) {
  d[0] = finish_word(mode, a2m, origin, 0, 0, false);
  d[1] = finish_word(mode, a2m, origin, 0, 0, true);
  d[2] = kBypassWord;
}
// A column whose word is the same whatever the request (initialisation error, group expression that
// is not a bool): that word first.
inline void packed_dict_const(uint32_t word, uint32_t d[3]) {
  d[0] = d[1] = word;
  d[2] = kBypassWord;
}

// How a wave of the pack kernels covers items: a lane holds one column of one item; an item takes
// `w` lanes (its columns: 64, or npol where npol <= 32 and a wave then takes ipi = 64 / npol items a
// round); a wave runs T rounds, so ipw = ipi * T consecutive items, and lane j < ipw ends up holding
// item j's planes: the plane stores of a wave are ipw contiguous 16-byte words.
struct PackGeom {
  uint32_t w, ipi, T, ipw;
};
KW_HD inline PackGeom pack_geom(uint32_t npol) {
  PackGeom g;
  g.w = npol <= 32u ? npol : 64u;
  g.ipi = 64u / g.w;
  g.T = 64u / g.ipi < 16u ? 64u / g.ipi : 16u;
  g.ipw = g.ipi * g.T;
  return g;
}
// The offsets scan (reports.hip): a workgroup of 256 threads scans kScanPer counts per thread.
constexpr uint32_t kScanPer = 4, kScanBlock = 256 * kScanPer;

KW_HD inline uint32_t packed_popc(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }
KW_HD inline uint64_t packed_below(uint32_t c) { return c ? ~0ull >> (64u - c) : 0ull; }  // bits [0, c), c < 64

// The reference encoder: words [rows][npol] under p->dict into p->planes, p->exc_off and p->exc.
// Exceptions beyond p->exc_cap are counted, not stored: KW_E_NOSPACE with the need in p->exc_count
// (the arrays' contents are then unspecified).
inline int packed_encode(const uint32_t* words, kw_packed* p) {
  if (!p || !packed_fits(p->rows, p->npol) || !p->dict || !p->exc_off) return KW_E_ARG;
  if (p->rows && (!words || !p->planes)) return KW_E_ARG;
  const uint32_t G = packed_groups(p->npol);
  size_t n = 0;
  for (uint64_t r = 0; r < p->rows; ++r) {
    p->exc_off[r] = (uint32_t)n;
    for (uint32_t g = 0; g < G; ++g) {
      uint64_t lo = 0, hi = 0;
      for (uint32_t c = 0; c < 64u && 64u * g + c < p->npol; ++c) {
        const uint32_t col = 64u * g + c, w = words[r * p->npol + col];
        const uint32_t code = packed_code(w, p->dict[3 * col], p->dict[3 * col + 1], p->dict[3 * col + 2]);
        lo |= (uint64_t)(code & 1u) << c;
        hi |= (uint64_t)(code >> 1) << c;
        if (code == kPackEscape) {
          if (n < p->exc_cap && p->exc) p->exc[n] = w;
          ++n;
        }
      }
      p->planes[2 * (r * G + g)] = lo;
      p->planes[2 * (r * G + g) + 1] = hi;
    }
  }
  p->exc_off[p->rows] = (uint32_t)n;
  p->exc_count = n;
  return n > p->exc_cap ? KW_E_NOSPACE : KW_OK;
}

// The word of (row, col): its dictionary entry, or exception number exc_off[row] + the escape bits
// of the row below col.
inline int packed_word(const kw_packed* p, uint64_t row, uint32_t col, uint32_t* word) {
  if (!p || !word || row >= p->rows || col >= p->npol) return KW_E_ARG;
  const uint32_t G = packed_groups(p->npol), g = col / 64u, c = col % 64u;
  const uint64_t* pl = p->planes + 2 * (row * G);
  const uint32_t code = (uint32_t)((pl[2 * g] >> c) & 1u) | ((uint32_t)((pl[2 * g + 1] >> c) & 1u) << 1);
  if (code != kPackEscape) {
    *word = p->dict[3 * col + code];
    return KW_OK;
  }
  size_t at = p->exc_off[row];
  for (uint32_t q = 0; q < g; ++q) at += packed_popc(pl[2 * q] & pl[2 * q + 1]);
  at += packed_popc(pl[2 * g] & pl[2 * g + 1] & packed_below(c));
  if (at >= p->exc_count || at >= p->exc_cap) return KW_E_ARG;
  *word = p->exc[at];
  return KW_OK;
}

// Rows [row0, row1) as full words, out [row1 - row0][npol].
inline int packed_unpack(const kw_packed* p, uint64_t row0, uint64_t row1, uint32_t* out) {
  if (!p || row0 > row1 || row1 > p->rows || (!out && row1 > row0)) return KW_E_ARG;
  const uint32_t G = packed_groups(p->npol);
  for (uint64_t r = row0; r < row1; ++r) {
    size_t at = p->exc_off[r];
    uint32_t* o = out + (r - row0) * p->npol;
    for (uint32_t g = 0; g < G; ++g) {
      const uint64_t lo = p->planes[2 * (r * G + g)], hi = p->planes[2 * (r * G + g) + 1];
      for (uint32_t c = 0; c < 64u && 64u * g + c < p->npol; ++c) {
        const uint32_t col = 64u * g + c, code = (uint32_t)((lo >> c) & 1u) | ((uint32_t)((hi >> c) & 1u) << 1);
        if (code != kPackEscape) {
          o[col] = p->dict[3 * col + code];
        } else {
          if (at >= p->exc_count || at >= p->exc_cap) return KW_E_ARG;
          o[col] = p->exc[at++];
        }
      }
    }
  }
  return KW_OK;
}

}  // namespace kw
