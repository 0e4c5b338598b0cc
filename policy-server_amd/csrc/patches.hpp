// patches.hpp — the pure arithmetic of the JSONPatch of an accepted mutation (include/kwgpu.h
// kw_batch_patches): what capabilities_patch (service.cpp) cuts from the document, restated over the
// columns. Per container, in batch order: the required drops that no string of its drop range
// equals (none when the range holds ALL), the default adds that are in neither range, and the ops
// the container's shape code selects (one adding securityContext, one adding capabilities, a whole
// add or drop list, or one .../add/- or .../drop/- op per name, adds first), under the path the
// request's pointer, the list's name and the item's index give.
//
// The shape: the ops text is produced by one walk (patch_walk) that hands every span to a PatchOut,
// which keeps the bytes of [skip, end) and counts the rest. patch_measure is the walk with an empty
// range, patch_render_window the walk with the window's. Nothing is kept between spans but scalars: a
// container's missing sets are recomputed where they are needed (counted, then listed), so there is
// no array a lane would index at run time. The response form wraps base64(ops) in the envelope;
// patch_response_window renders the raw bytes under the window's quads into a side buffer and
// encodes from there, for any skip. Every function the device runs is KW_HD; no HIP, no batch, no
// settings of the process (tests/patches_check.cpp runs it on the host).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "responses.hpp"

namespace kw {

// ---- the literals of the ops and of the envelope, each once ------------------------------------------
#define KW_PATCH_LITS(X)                                                          \
  X(PL_OP, "{\"op\":\"add\",\"path\":\"")                                         \
  X(PL_VALUE, "\",\"value\":")                                                    \
  X(PL_POD, "/spec")                                                              \
  X(PL_TEMPLATE, "/spec/template/spec")                                           \
  X(PL_CRONJOB, "/spec/jobTemplate/spec/template/spec")                           \
  X(PL_CONTAINERS, "/containers/")                                                \
  X(PL_INIT, "/initContainers/")                                                  \
  X(PL_EPHEMERAL, "/ephemeralContainers/")                                        \
  X(PL_SC, "/securityContext")                                                    \
  X(PL_CAPS, "/capabilities")                                                     \
  X(PL_ADD, "/add")                                                               \
  X(PL_DROP, "/drop")                                                             \
  X(PL_DASH, "/-")                                                                \
  X(PL_CAPOBJ, "{\"capabilities\":")                                              \
  X(PL_KADD, "\"add\":[")                                                         \
  X(PL_KDROP, "\"drop\":[")                                                       \
  X(PL_ALL, "ALL")                                                                \
  X(PL_R_OPEN, "{\"uid\":\"")                                                     \
  X(PL_R_MID, "\",\"allowed\":true,\"patchType\":\"JSONPatch\",\"patch\":\"")     \
  X(PL_R_END, "\"}")

enum PatchLit : uint32_t {
#define X(id, s) id##_AT, id##_LAST = id##_AT + sizeof(s) - 2,
  KW_PATCH_LITS(X)
#undef X
  PL_BYTES
};
enum : uint32_t {
#define X(id, s) id##_LEN = sizeof(s) - 1,
  KW_PATCH_LITS(X)
#undef X
};
#define X(id, s) s
constexpr char kPatchLitText[] = KW_PATCH_LITS(X);
#undef X
static_assert(sizeof(kPatchLitText) - 1 == PL_BYTES, "the literals' places add up to the table");

// ---- the settings table --------------------------------------------------------------------------------
// One block: [PatchHead][PatchCol x ncols][PatchName x nnames][text]. The text starts with
// kPatchLitText; a name is held raw (compared with the columns' strings) and JSON-escaped between
// quotes (copied). A column's names: its required drops, then its default adds, each list
// de-duplicated in settings order as capabilities_patch's uniq does it.
enum : uint32_t { PC_CAPABILITIES = 1u };
struct PatchCol {
  uint32_t flags;
  uint32_t req_at, nreq;  // required drops
  uint32_t def_at, ndef;  // default adds
};
struct PatchName {
  MsgSpan raw, esc;
};
struct PatchHead {
  uint32_t ncols, nnames, text_bytes, bytes;
};
struct PatchSettings {
  const PatchCol* col;
  const PatchName* name;
  const uint8_t* text;
  uint32_t ncols;
};
KW_HD inline PatchSettings patch_settings(const uint8_t* block) {
  const PatchHead* h = (const PatchHead*)block;
  PatchSettings S;
  S.ncols = h->ncols;
  S.col = (const PatchCol*)(block + sizeof(PatchHead));
  S.name = (const PatchName*)(S.col + h->ncols);
  S.text = (const uint8_t*)(S.name + h->nnames);
  return S;
}

// What the host hands over per column (patches.cpp fills it from PolicyRec); every string raw.
struct PatchColSource {
  bool capabilities = false;
  std::vector<std::string> required_drop, default_add;
};
inline std::vector<uint64_t> patch_build_table(const std::vector<PatchColSource>& cols) {
  std::string text(kPatchLitText, PL_BYTES);
  std::vector<PatchCol> C;
  std::vector<PatchName> N;
  auto put = [&](const std::string& s) {
    MsgSpan sp{(uint32_t)text.size(), (uint32_t)s.size()};
    text += s;
    return sp;
  };
  auto names = [&](const std::vector<std::string>& l, uint32_t* at, uint32_t* n) {
    *at = (uint32_t)N.size();
    std::vector<std::string> seen;
    for (const std::string& x : l) {
      bool dup = false;
      for (const std::string& y : seen) dup = dup || y == x;
      if (dup) continue;
      seen.push_back(x);
      PatchName pn;
      pn.raw = put(x);
      pn.esc = put("\"" + rsp_escaped(x) + "\"");
      N.push_back(pn);
    }
    *n = (uint32_t)N.size() - *at;
  };
  for (const PatchColSource& s : cols) {
    PatchCol c{};
    c.flags = s.capabilities ? PC_CAPABILITIES : 0u;
    if (s.capabilities) {
      names(s.required_drop, &c.req_at, &c.nreq);
      names(s.default_add, &c.def_at, &c.ndef);
    }
    C.push_back(c);
  }
  const size_t bytes = sizeof(PatchHead) + C.size() * sizeof(PatchCol) + N.size() * sizeof(PatchName) + text.size();
  PatchHead h{(uint32_t)C.size(), (uint32_t)N.size(), (uint32_t)text.size(), (uint32_t)bytes};
  std::vector<uint64_t> block((bytes + 7) / 8 + 1, 0);
  uint8_t* p = (uint8_t*)block.data();
  memcpy(p, &h, sizeof(h));
  p += sizeof(h);
  if (!C.empty()) memcpy(p, C.data(), C.size() * sizeof(PatchCol));
  p += C.size() * sizeof(PatchCol);
  if (!N.empty()) memcpy(p, N.data(), N.size() * sizeof(PatchName));
  p += N.size() * sizeof(PatchName);
  memcpy(p, text.data(), text.size());
  return block;
}

// ---- the columns -----------------------------------------------------------------------------------------
// Batch rows on the host, device rows on the device; a string column that is not resident has off
// = nullptr.
struct PatchCols {
  uint64_t rows, nctr;
  const uint32_t *ctr_off, *capadd_off, *capdrop_off;
  const uint8_t* ctr_flags;
  DigestStr add, drop, uid;
  const uint32_t* ctr_place;  // [nctr] KW_PS_PLACE
  const uint8_t* req_place;   // [rows] KW_PP_*
};
struct PatchCtx {
  PatchCols C;
  PatchSettings S;
};
enum PatchStatus : uint32_t { PATCH_TEXT = 0, PATCH_HOST = 1, PATCH_MISSING = 2 };

// The rules of the header: PATCH_HOST for an item this renderer leaves to the host, PATCH_MISSING
// when a column it reads is not resident. col < S.ncols is the caller's check.
KW_HD inline uint32_t patch_item(const PatchCtx& X, uint64_t row, uint32_t col, uint32_t word, uint32_t form) {
  const PatchCols& C = X.C;
  if (!(word & KW_F_PATCH) || !(X.S.col[col].flags & PC_CAPABILITIES)) return PATCH_HOST;
  if (!C.add.off || !C.drop.off || !C.ctr_place || !C.req_place || (form == (uint32_t)KW_PATCH_RESPONSE && !C.uid.off))
    return PATCH_MISSING;
  if (row >= C.rows || (form == (uint32_t)KW_PATCH_RESPONSE && row >= C.uid.n)) return PATCH_HOST;
  if (C.req_place[row] == (uint8_t)KW_PP_UNKNOWN || C.req_place[row] > (uint8_t)KW_PP_CRONJOB) return PATCH_HOST;
  const uint32_t cb = C.ctr_off[row], ce = C.ctr_off[row + 1];
  if (ce < cb || ce > C.nctr) return PATCH_HOST;
  for (uint32_t c = cb; c < ce; ++c) {
    const uint32_t shape = KW_PS_SHAPE(C.ctr_place[c]);
    if (shape == (uint32_t)KW_PS_UNKNOWN || shape > (uint32_t)KW_PS_MAX) return PATCH_HOST;
    if (C.capadd_off[c + 1] < C.capadd_off[c] || C.capadd_off[c + 1] > C.add.n || C.capdrop_off[c + 1] < C.capdrop_off[c] ||
        C.capdrop_off[c + 1] > C.drop.n)
      return PATCH_HOST;
  }
  return PATCH_TEXT;
}

// ---- the output: the bytes of [skip, end) kept, the others counted ----------------------------------------
struct PatchOut {
  uint32_t at;         // the place of the next byte in the text
  uint32_t skip, end;  // the range kept (end = 0: none, the walk measures)
  uint8_t* dst;        // where byte `skip` goes
};
KW_HD inline bool po_done(const PatchOut& o) { return o.end != 0u && o.at >= o.end; }
KW_HD inline void po_put(PatchOut& o, const uint8_t* p, uint32_t n) {
  const uint32_t a = o.at, b = a + n;
  o.at = b;
  if (b <= o.skip || a >= o.end) return;
  const uint32_t lo = a > o.skip ? a : o.skip, hi = b < o.end ? b : o.end;
  rsp_copy_raw(p + (lo - a), hi - lo, o.dst + (lo - o.skip));
}
KW_HD inline void po_putc(PatchOut& o, char c) {
  const uint32_t a = o.at++;
  if (a >= o.skip && a < o.end) o.dst[a - o.skip] = (uint8_t)c;
}
#define KW_PATCH_LIT(o, S, id) po_put((o), (S).text + id##_AT, id##_LEN)
// The decimal digits of v.
KW_HD inline void po_dec(PatchOut& o, uint32_t v) {
  uint32_t p = 1;
  while (v / p >= 10u) p *= 10u;
  for (; p; p /= 10u) po_putc(o, (char)('0' + (v / p) % 10u));
}

// ---- a container's missing sets ------------------------------------------------------------------------------
KW_HD inline bool patch_has(const DigestStr& s, uint32_t b, uint32_t e, const uint8_t* p, uint32_t n) {
  for (uint32_t k = b; k < e; ++k) {
    const uint32_t a = s.off[k];
    if (s.off[k + 1] - a != n) continue;
    uint32_t i = 0;
    while (i < n && s.bytes[a + i] == p[i]) ++i;
    if (i == n) return true;
  }
  return false;
}
struct PatchCtr {
  uint32_t ab, ae, db, de;  // the container's add and drop ranges
  bool has_all;             // its drop range holds ALL
};
// Whether name j of the column's list (which 0: default adds, 1: required drops) is missing from
// the container.
KW_HD inline bool patch_missing(const PatchCtx& X, const PatchCol& pc, const PatchCtr& k, uint32_t which, uint32_t j) {
  const PatchName& nm = X.S.name[(which ? pc.req_at : pc.def_at) + j];
  const uint8_t* p = X.S.text + nm.raw.at;
  if (which) return !k.has_all && !patch_has(X.C.drop, k.db, k.de, p, nm.raw.n);
  return !patch_has(X.C.add, k.ab, k.ae, p, nm.raw.n) && !patch_has(X.C.drop, k.db, k.de, p, nm.raw.n);
}
KW_HD inline uint32_t patch_count(const PatchCtx& X, const PatchCol& pc, const PatchCtr& k, uint32_t which) {
  uint32_t n = 0;
  for (uint32_t j = 0, e = which ? pc.nreq : pc.ndef; j < e; ++j) n += patch_missing(X, pc, k, which, j) ? 1u : 0u;
  return n;
}
// ["a","b"]: the missing names of one list.
KW_HD inline void patch_list(const PatchCtx& X, const PatchCol& pc, const PatchCtr& k, uint32_t which, PatchOut& o) {
  po_putc(o, '[');
  bool first = true;
  for (uint32_t j = 0, e = which ? pc.nreq : pc.ndef; j < e; ++j) {
    if (!patch_missing(X, pc, k, which, j)) continue;
    if (!first) po_putc(o, ',');
    first = false;
    const PatchName& nm = X.S.name[(which ? pc.req_at : pc.def_at) + j];
    po_put(o, X.S.text + nm.esc.at, nm.esc.n);
  }
  po_putc(o, ']');
}
// {"add":[...],"drop":[...]} with the lists that are not empty.
KW_HD inline void patch_capobj(const PatchCtx& X, const PatchCol& pc, const PatchCtr& k, uint32_t nadd, uint32_t ndrop, PatchOut& o) {
  po_putc(o, '{');
  if (nadd) {
    po_put(o, X.S.text + PL_KADD_AT, PL_KADD_LEN - 1u);  // (patch_list opens the bracket)
    patch_list(X, pc, k, 0u, o);
  }
  if (ndrop) {
    if (nadd) po_putc(o, ',');
    po_put(o, X.S.text + PL_KDROP_AT, PL_KDROP_LEN - 1u);
    patch_list(X, pc, k, 1u, o);
  }
  po_putc(o, '}');
}
// The opening of an op up to .../securityContext: the separator, {"op":"add","path":"<pointer>/<list>/<index>/securityContext
KW_HD inline void patch_op(const PatchCtx& X, uint32_t pointer, uint32_t flags, uint32_t index, bool* first, PatchOut& o) {
  const PatchSettings& S = X.S;
  if (!*first) po_putc(o, ',');
  *first = false;
  KW_PATCH_LIT(o, S, PL_OP);
  if (pointer == (uint32_t)KW_PP_POD) KW_PATCH_LIT(o, S, PL_POD);
  else if (pointer == (uint32_t)KW_PP_TEMPLATE) KW_PATCH_LIT(o, S, PL_TEMPLATE);
  else KW_PATCH_LIT(o, S, PL_CRONJOB);
  if (flags & KW_CTR_INIT) KW_PATCH_LIT(o, S, PL_INIT);
  else if (flags & KW_CTR_EPHEMERAL) KW_PATCH_LIT(o, S, PL_EPHEMERAL);
  else KW_PATCH_LIT(o, S, PL_CONTAINERS);
  po_dec(o, index);
  KW_PATCH_LIT(o, S, PL_SC);
}

// The ops text of (row, col), an item patch_item called PATCH_TEXT, into o.
KW_HD inline void patch_walk(const PatchCtx& X, uint64_t row, uint32_t col, PatchOut& o) {
  const PatchCols& C = X.C;
  const PatchSettings& S = X.S;
  const PatchCol& pc = S.col[col];
  const uint32_t pointer = C.req_place[row];
  po_putc(o, '[');
  bool first = true;
  const uint32_t cb = C.ctr_off[row], ce = pointer == (uint32_t)KW_PP_NONE ? cb : C.ctr_off[row + 1];
  for (uint32_t c = cb; c < ce && !po_done(o); ++c) {
    PatchCtr k;
    k.ab = C.capadd_off[c], k.ae = C.capadd_off[c + 1];
    k.db = C.capdrop_off[c], k.de = C.capdrop_off[c + 1];
    k.has_all = patch_has(C.drop, k.db, k.de, S.text + PL_ALL_AT, PL_ALL_LEN);
    const uint32_t ndrop = patch_count(X, pc, k, 1u), nadd = patch_count(X, pc, k, 0u);
    if (!ndrop && !nadd) continue;
    const uint32_t place = C.ctr_place[c], shape = KW_PS_SHAPE(place), index = KW_PS_INDEX(place), flags = C.ctr_flags[c];
    if (shape == (uint32_t)KW_PS_NO_SC) {
      patch_op(X, pointer, flags, index, &first, o);
      KW_PATCH_LIT(o, S, PL_VALUE);
      KW_PATCH_LIT(o, S, PL_CAPOBJ);
      patch_capobj(X, pc, k, nadd, ndrop, o);
      po_putc(o, '}');
      po_putc(o, '}');
      continue;
    }
    if (shape == (uint32_t)KW_PS_NO_CAPS) {
      patch_op(X, pointer, flags, index, &first, o);
      KW_PATCH_LIT(o, S, PL_CAPS);
      KW_PATCH_LIT(o, S, PL_VALUE);
      patch_capobj(X, pc, k, nadd, ndrop, o);
      po_putc(o, '}');
      continue;
    }
    for (uint32_t which = 0; which < 2u; ++which) {  // adds before drops
      if (!(which ? ndrop : nadd)) continue;
      const bool is_arr = ((shape - (uint32_t)KW_PS_CAPS) & (which ? (uint32_t)KW_PS_DROP_ARRAY : (uint32_t)KW_PS_ADD_ARRAY)) != 0u;
      if (!is_arr) {
        patch_op(X, pointer, flags, index, &first, o);
        KW_PATCH_LIT(o, S, PL_CAPS);
        if (which) KW_PATCH_LIT(o, S, PL_DROP);
        else KW_PATCH_LIT(o, S, PL_ADD);
        KW_PATCH_LIT(o, S, PL_VALUE);
        patch_list(X, pc, k, which, o);
        po_putc(o, '}');
        continue;
      }
      for (uint32_t j = 0, e = which ? pc.nreq : pc.ndef; j < e && !po_done(o); ++j) {
        if (!patch_missing(X, pc, k, which, j)) continue;
        patch_op(X, pointer, flags, index, &first, o);
        KW_PATCH_LIT(o, S, PL_CAPS);
        if (which) KW_PATCH_LIT(o, S, PL_DROP);
        else KW_PATCH_LIT(o, S, PL_ADD);
        KW_PATCH_LIT(o, S, PL_DASH);
        KW_PATCH_LIT(o, S, PL_VALUE);
        const PatchName& nm = S.name[(which ? pc.req_at : pc.def_at) + j];
        po_put(o, S.text + nm.esc.at, nm.esc.n);
        po_putc(o, '}');
      }
    }
  }
  if (!po_done(o)) po_putc(o, ']');
}

// The length of the ops text.
KW_HD inline uint32_t patch_measure(const PatchCtx& X, uint64_t row, uint32_t col) {
  PatchOut o{0u, 0u, 0u, nullptr};
  patch_walk(X, row, col, o);
  return o.at;
}
// Writes bytes [skip, skip + n) of the ops text to dst; the caller keeps skip + n within the length.
KW_HD inline void patch_render_window(const PatchCtx& X, uint64_t row, uint32_t col, uint32_t skip, uint32_t n, uint8_t* dst) {
  if (!n) return;
  PatchOut o{0u, skip, skip + n, dst};
  patch_walk(X, row, col, o);
}

// ---- the response form ------------------------------------------------------------------------------------------
KW_HD inline uint32_t patch_b64_len(uint32_t l) { return 4u * ((l + 2u) / 3u); }
KW_HD inline uint8_t patch_b64_char(uint32_t v) {
  if (v < 26u) return (uint8_t)('A' + v);
  if (v < 52u) return (uint8_t)('a' + (v - 26u));
  if (v < 62u) return (uint8_t)('0' + (v - 52u));
  return (uint8_t)(v == 62u ? '+' : '/');
}
// The envelope's head: {"uid":"<escaped uid>","allowed":true,"patchType":"JSONPatch","patch":"
struct PatchEnvelope {
  const uint8_t* uid;
  uint32_t un, ue;  // the uid's raw and escaped length
  uint32_t head;    // the head's length
};
KW_HD inline PatchEnvelope patch_envelope(const PatchCtx& X, uint64_t row) {
  PatchEnvelope e;
  e.uid = nullptr;
  e.un = 0;
  (void)msg_entity(X.C.uid, row, &e.uid, &e.un);
  e.ue = rsp_esc_len(e.uid, e.un);
  e.head = PL_R_OPEN_LEN + e.ue + PL_R_MID_LEN;
  return e;
}
// The response's length for an ops text of l bytes.
KW_HD inline uint32_t patch_response_len(const PatchEnvelope& e, uint32_t l) { return e.head + patch_b64_len(l) + PL_R_END_LEN; }
// The bytes of the side buffer a render of n output bytes may need: the raw bytes under the quads
// that n base64 characters touch at any phase.
KW_HD inline uint32_t patch_raw_need(uint32_t n) { return 3u * ((n + 6u) / 4u); }

// Writes bytes [skip, skip + n) of the response to dst; l: the ops text's length (patch_measure).
// The base64 characters inside the range are cut from whole quads counted from the start of the
// item's base64 text: the raw bytes under those quads are rendered into `raw` (patch_raw_need(n)
// bytes), the characters computed from there, '=' where the ops text ends inside a quad.
KW_HD inline void patch_response_window(const PatchCtx& X, uint64_t row, uint32_t col, const PatchEnvelope& e, uint32_t l, uint32_t skip,
                                        uint32_t n, uint8_t* dst, uint8_t* raw) {
  if (!n) return;
  const PatchSettings& S = X.S;
  const uint32_t end = skip + n, nb = patch_b64_len(l), b_at = e.head, t_at = e.head + nb;
  PatchOut o{0u, skip, end, dst};
  KW_PATCH_LIT(o, S, PL_R_OPEN);
  if (o.at + e.ue > skip && o.at < end) {  // the part of the escaped uid inside the range
    const uint32_t lo = skip > o.at ? skip - o.at : 0u, hi = end - o.at < e.ue ? end - o.at : e.ue;
    rsp_esc_write(e.uid, e.un, lo, hi - lo, dst + (o.at + lo - skip));
  }
  o.at += e.ue;
  KW_PATCH_LIT(o, S, PL_R_MID);
  const uint32_t b0 = (skip > b_at ? skip : b_at) - b_at, b1 = (end < t_at ? end : t_at) > b_at ? (end < t_at ? end : t_at) - b_at : 0u;
  if (b1 > b0) {
    const uint32_t q0 = b0 / 4u, q1 = (b1 + 3u) / 4u, r0 = 3u * q0, r1 = 3u * q1 < l ? 3u * q1 : l;
    patch_render_window(X, row, col, r0, r1 - r0, raw);
    uint8_t* d = dst + (b_at + b0 - skip);
    for (uint32_t g = b0; g < b1; ++g) {
      const uint32_t i = 3u * (g / 4u), k = g & 3u;
      const uint32_t x0 = raw[i - r0], x1 = i + 1u < l ? raw[i + 1u - r0] : 0u, x2 = i + 2u < l ? raw[i + 2u - r0] : 0u;
      uint8_t ch;
      if (k == 0u) ch = patch_b64_char(x0 >> 2);
      else if (k == 1u) ch = patch_b64_char(((x0 & 3u) << 4) | (x1 >> 4));
      else if (k == 2u) ch = i + 1u < l ? patch_b64_char(((x1 & 15u) << 2) | (x2 >> 6)) : (uint8_t)'=';
      else ch = i + 2u < l ? patch_b64_char(x2 & 63u) : (uint8_t)'=';
      d[g - b0] = ch;
    }
  }
  o.at = t_at;
  KW_PATCH_LIT(o, S, PL_R_END);
}

// One item's status and length in `form` (what the length kernel and the host renderer compute).
KW_HD inline uint32_t patch_length(const PatchCtx& X, uint64_t row, uint32_t col, uint32_t word, uint32_t form, uint32_t* len) {
  *len = 0;
  const uint32_t st = patch_item(X, row, col, word, form);
  if (st != (uint32_t)PATCH_TEXT) return st;
  const uint32_t l = patch_measure(X, row, col);
  *len = form == (uint32_t)KW_PATCH_RESPONSE ? patch_response_len(patch_envelope(X, row), l) : l;
  return PATCH_TEXT;
}

}  // namespace kw
