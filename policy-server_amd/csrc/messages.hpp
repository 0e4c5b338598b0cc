// messages.hpp — the pure arithmetic of the messages of chosen findings (include/kwgpu.h
// kw_batch_messages): the text policy_message (service.cpp) gives for one pair of a pass, cut into
// pieces. A piece is a span of bytes: a literal fragment of the one table below, a string of a
// request column or of the container-name column, or a string of the pass's settings table (the
// valid namespace, a mandatory key, a constraint's regex, a group's message, an initialisation
// error). message_pieces gives the pieces of one item or says "host"; msg_copy_window writes the
// part of a message that falls into one window of the output, msg_clip and msg_chunks are the
// window and alignment arithmetic of the write kernel (reports.hip messages_write_kernel), and
// MsgTable is the settings table as the host builds it. Every function the device runs is KW_HD:
// the host renderer (kw_debug_messages_words how = 1) runs the same code over the host columns.
// No HIP, no batch, no settings of the process (tests/messages_check.cpp runs it on the host).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "digest.hpp"
#include "imgscan.hpp"

namespace kw {

// ---- the literal fragments: the texts of policy_message, each once -----------------------------
// X(id, text); no text is empty. The table travels at the head of the settings table's bytes, so a
// literal piece is a span like any other.
#define KW_MSG_LITS(X)                                          \
  X(ML_PRIVILEGED, "Privileged container is not allowed")       \
  X(ML_NS_HEAD, "namespace '")                                  \
  X(ML_NS_MID, "' is not accepted: only '")                     \
  X(ML_NS_TAIL, "' is allowed")                                 \
  X(ML_CTR, "container '")                                      \
  X(ML_USES_IMAGE, "' uses image '")                            \
  X(ML_REGISTRY, "': registry '")                               \
  X(ML_TAG, "': tag '")                                         \
  X(ML_NOT_ALLOWED_REG, "' is not in the allowed registries")   \
  X(ML_IS_REJECTED, "' is rejected")                            \
  X(ML_NOT_ALLOWED_IMG, "', which is not in the allowed images") \
  X(ML_WHICH_REJECTED, "', which is rejected")                  \
  X(ML_ADDS_CAP, "' adds capability '")                         \
  X(ML_WHICH_NOT_ALLOWED, "', which is not allowed")            \
  X(ML_USES_AA, "' uses AppArmor profile '")                    \
  X(ML_LABEL, "label '")                                        \
  X(ML_IS_DENIED, "' is denied")                                \
  X(ML_VALUE, "' value '")                                      \
  X(ML_CONSTRAINT, "' does not match the constraint '")         \
  X(ML_QUOTE, "'")                                              \
  X(ML_MANDATORY, "mandatory label '")                          \
  X(ML_IS_MISSING, "' is missing")                              \
  X(ML_DOCKER_IO, "docker.io")                                  \
  X(ML_LATEST, "latest")

// id##_AT: the fragment's place in kMsgLitText (an enumerator follows its predecessor by one, so the
// next fragment starts one past id##_LAST); id##_LEN its length.
enum MsgLit : uint32_t {
#define X(id, s) id##_AT, id##_LAST = id##_AT + sizeof(s) - 2,
  KW_MSG_LITS(X)
#undef X
  ML_BYTES
};
enum : uint32_t {
#define X(id, s) id##_LEN = sizeof(s) - 1,
  KW_MSG_LITS(X)
#undef X
};
#define X(id, s) s
constexpr char kMsgLitText[] = KW_MSG_LITS(X);
#undef X
static_assert(sizeof(kMsgLitText) - 1 == ML_BYTES, "the fragments' places add up to the table");

// ---- the settings table of a pass ---------------------------------------------------------------
// One block of bytes, built per call from (env, policies): [MsgHead][MsgCol x ncols][MsgSpan x
// mandatory keys][MsgCons x constrained keys][text]. Every span is (offset into text, length); the
// text starts with kMsgLitText.
struct MsgSpan {
  uint32_t at, n;
};
struct MsgCons {  // a constrained key and its regex text
  MsgSpan key, re;
};
struct MsgCol {
  uint32_t family;
  MsgSpan ns;             // valid_namespace ("" when the list is empty)
  MsgSpan message, init;  // P.message, P.init_message
  uint32_t mand_at, nmand;  // the mandatory keys, settings order
  uint32_t cons_at, ncons;  // the constrained keys, ordered by msg_key_less
};
struct MsgHead {
  uint32_t ncols, nmand, ncons, text_bytes;
};
// The table as the functions below read it (pointers into one block, host or device).
struct MsgSettings {
  const MsgCol* col;
  const MsgSpan* mand;
  const MsgCons* cons;
  const uint8_t* text;
  uint32_t ncols;
};
KW_HD inline MsgSettings msg_settings(const uint8_t* block) {
  const MsgHead* h = (const MsgHead*)block;
  MsgSettings S;
  S.ncols = h->ncols;
  S.col = (const MsgCol*)(block + sizeof(MsgHead));
  S.mand = (const MsgSpan*)(S.col + h->ncols);
  S.cons = (const MsgCons*)(S.mand + h->nmand);
  S.text = (const uint8_t*)(S.cons + h->ncons);
  return S;
}

// The order of the constrained keys: by length, then by bytes. <0, 0, >0.
KW_HD inline int msg_key_cmp(const uint8_t* a, uint32_t na, const uint8_t* b, uint32_t nb) {
  if (na != nb) return na < nb ? -1 : 1;
  for (uint32_t i = 0; i < na; ++i)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return 0;
}
// The first entry of column c whose key equals (k, n), or 0xffffffff: a binary search for the lower
// bound (equal keys keep settings order, so the first is the entry policy_message finds).
KW_HD inline uint32_t msg_find_constraint(const MsgSettings& S, const MsgCol& c, const uint8_t* k, uint32_t n) {
  uint32_t lo = 0, hi = c.ncons;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    const MsgCons& e = S.cons[c.cons_at + mid];
    if (msg_key_cmp(S.text + e.key.at, e.key.n, k, n) < 0) lo = mid + 1u;
    else hi = mid;
  }
  if (lo < c.ncons) {
    const MsgCons& e = S.cons[c.cons_at + lo];
    if (msg_key_cmp(S.text + e.key.at, e.key.n, k, n) == 0) return c.cons_at + lo;
  }
  return 0xffffffffu;
}

// What the host hands over per column (messages.cpp fills it from PolicyRec).
struct MsgColSource {
  uint32_t family = 0;
  std::string ns, message, init;
  std::vector<std::string> mandatory, keys, regexes;  // keys[i] is constrained by regexes[i]
};
// The table's block (8-byte aligned storage).
inline std::vector<uint64_t> msg_build_table(const std::vector<MsgColSource>& cols) {
  std::string text(kMsgLitText, ML_BYTES);
  auto put = [&](const std::string& s) {
    MsgSpan sp{(uint32_t)text.size(), (uint32_t)s.size()};
    text += s;
    return sp;
  };
  std::vector<MsgCol> C;
  std::vector<MsgSpan> M;
  std::vector<MsgCons> K;
  for (const MsgColSource& s : cols) {
    MsgCol c{};
    c.family = s.family;
    c.ns = put(s.ns);
    c.message = put(s.message);
    c.init = put(s.init);
    c.mand_at = (uint32_t)M.size();
    c.nmand = (uint32_t)s.mandatory.size();
    for (const std::string& m : s.mandatory) M.push_back(put(m));
    const size_t nk = std::min(s.keys.size(), s.regexes.size());
    std::vector<uint32_t> order(nk);
    for (size_t i = 0; i < nk; ++i) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
      return msg_key_cmp((const uint8_t*)s.keys[a].data(), (uint32_t)s.keys[a].size(), (const uint8_t*)s.keys[b].data(),
                         (uint32_t)s.keys[b].size()) < 0;
    });
    c.cons_at = (uint32_t)K.size();
    c.ncons = (uint32_t)nk;
    for (uint32_t i : order) {
      MsgCons e;
      e.key = put(s.keys[i]);
      e.re = put(s.regexes[i]);
      K.push_back(e);
    }
    C.push_back(c);
  }
  MsgHead h{(uint32_t)C.size(), (uint32_t)M.size(), (uint32_t)K.size(), (uint32_t)text.size()};
  const size_t bytes = sizeof(MsgHead) + C.size() * sizeof(MsgCol) + M.size() * sizeof(MsgSpan) + K.size() * sizeof(MsgCons) + text.size();
  std::vector<uint64_t> block((bytes + 16 + 7) / 8, 0);  // (a zero tail, as the string pools have)
  uint8_t* p = (uint8_t*)block.data();
  memcpy(p, &h, sizeof(h));
  p += sizeof(h);
  if (!C.empty()) memcpy(p, C.data(), C.size() * sizeof(MsgCol));
  p += C.size() * sizeof(MsgCol);
  if (!M.empty()) memcpy(p, M.data(), M.size() * sizeof(MsgSpan));
  p += M.size() * sizeof(MsgSpan);
  if (!K.empty()) memcpy(p, K.data(), K.size() * sizeof(MsgCons));
  p += K.size() * sizeof(MsgCons);
  memcpy(p, text.data(), text.size());
  return block;
}

// ---- the piece plan ------------------------------------------------------------------------------
constexpr uint32_t kMsgMaxPieces = 8;  // (reasons 3-5 and 11 take seven)
struct MsgPiece {
  const uint8_t* p;
  uint32_t n;
};
struct MsgPlan {
  MsgPiece pc[kMsgMaxPieces];
  uint32_t npc;
  uint32_t len;  // the sum of the pieces
};
enum MsgStatus : uint32_t {
  MSG_TEXT = 0,     // rendered (the empty message included)
  MSG_HOST = 1,     // left to the host: reason 14, a wide argument, an argument the request does not hold
  MSG_MISSING = 2   // a column the message quotes is not there (the call answers KW_E_ARG)
};
// The columns a message is cut from: the digest's (the pass's own) and the container names.
struct MsgCols {
  DigestCols c;
  DigestStr name;
};

// Piece k of the plan. Every call site names k as a constant, and msg_copy_window walks the places
// unrolled, so a kernel keeps the plan in registers (with a run-time place it lay in scratch, 144
// bytes a lane).
KW_HD inline void msg_set(MsgPlan* P, uint32_t k, const uint8_t* p, uint32_t n) {
  P->pc[k].p = p;
  P->pc[k].n = n;
  P->len += n;
}
// (tests: the next free place)
KW_HD inline void msg_put(MsgPlan* P, const uint8_t* p, uint32_t n) { msg_set(P, P->npc++, p, n); }
#define KW_MSG_LIT(P, k, S, id) msg_set((P), (k), (S).text + id##_AT, id##_LEN)
KW_HD inline void msg_set_span(MsgPlan* P, uint32_t k, const MsgSettings& S, MsgSpan s) { msg_set(P, k, S.text + s.at, s.n); }

// Whether the device renders a word at all (the rules of the header): 0 text, 1 host. A reason no
// product word has, and reason 0, render as the empty message.
KW_HD inline bool msg_word_host(uint32_t word) {
  const uint32_t r = KW_REASON(word);
  return r == (uint32_t)KW_R_GROUP_EXPR || (r >= 1u && r <= 12u && KW_ARG(word) == KW_ARG_WIDE);
}

// One string of a column as a piece; false when the column does not hold entity e.
KW_HD inline bool msg_entity(const DigestStr& s, uint64_t e, const uint8_t** p, uint32_t* n) {
  if (e >= s.n) return false;
  const uint32_t a = s.off[e], b = s.off[e + 1];
  *p = s.bytes + a;
  *n = b - a;
  return true;
}

// The pieces of the message of `word` at (row, col); row < C.c.rows and col < S.ncols are the
// caller's checks. On MSG_HOST and MSG_MISSING the plan is empty (length 0).
KW_HD inline uint32_t message_pieces(const MsgCols& C, const MsgSettings& S, uint64_t row, uint32_t col, uint32_t word,
                                     MsgPlan* P) {
  P->npc = 0;
  P->len = 0;
  if (msg_word_host(word)) return MSG_HOST;
  const uint32_t reason = KW_REASON(word), arg = KW_ARG(word);
  const MsgCol& pc = S.col[col];
  const uint8_t *p0 = nullptr, *p1 = nullptr, *pn = nullptr;
  uint32_t n0 = 0, n1 = 0, nn = 0;
  const DigestCols& D = C.c;
  switch (reason) {
    case KW_R_PRIVILEGED:
      KW_MSG_LIT(P, 0, S, ML_PRIVILEGED);
      P->npc = 1;
      return MSG_TEXT;
    case KW_R_NAMESPACE:
      if (!D.str[DG_NS].off) return MSG_MISSING;
      (void)msg_entity(D.str[DG_NS], row, &p0, &n0);  // (a row the column lacks reads as "")
      KW_MSG_LIT(P, 0, S, ML_NS_HEAD);
      msg_set(P, 1, p0, n0);
      KW_MSG_LIT(P, 2, S, ML_NS_MID);
      msg_set_span(P, 3, S, pc.ns);
      KW_MSG_LIT(P, 4, S, ML_NS_TAIL);
      P->npc = 5;
      return MSG_TEXT;
    case KW_R_REG_NOT_ALLOWED:
    case KW_R_REG_REJECTED:
    case KW_R_TAG_REJECTED:
    case KW_R_IMG_NOT_ALLOWED:
    case KW_R_IMG_REJECTED: {
      if (!D.str[DG_IMG].off || !C.name.off) return MSG_MISSING;
      const uint32_t cb = D.ctr_off[row], ce = D.ctr_off[row + 1];
      if (arg >= ce - cb || !msg_entity(C.name, (uint64_t)cb + arg, &pn, &nn) ||
          !msg_entity(D.str[DG_IMG], (uint64_t)cb + arg, &p0, &n0))
        return MSG_HOST;
      KW_MSG_LIT(P, 0, S, ML_CTR);
      msg_set(P, 1, pn, nn);
      KW_MSG_LIT(P, 2, S, ML_USES_IMAGE);
      msg_set(P, 3, p0, n0);
      if (reason == (uint32_t)KW_R_IMG_NOT_ALLOWED) {
        KW_MSG_LIT(P, 4, S, ML_NOT_ALLOWED_IMG);
        P->npc = 5;
        return MSG_TEXT;
      }
      if (reason == (uint32_t)KW_R_IMG_REJECTED) {
        KW_MSG_LIT(P, 4, S, ML_WHICH_REJECTED);
        P->npc = 5;
        return MSG_TEXT;
      }
      // the registry and the tag of image_parts (service.cpp), from the kernels' own scan
      const DigestStr& im = D.str[DG_IMG];
      const uint32_t b = im.off[(uint64_t)cb + arg], e = im.off[(uint64_t)cb + arg + 1];
      const ImageRef r = parse_image(im.bytes, b, e);
      P->npc = 7;
      if (reason == (uint32_t)KW_R_TAG_REJECTED) {
        KW_MSG_LIT(P, 4, S, ML_TAG);
        if (r.colon != 0xffffffffu) msg_set(P, 5, im.bytes + r.colon + 1u, r.name_end - (r.colon + 1u));
        else if (r.at == 0xffffffffu) KW_MSG_LIT(P, 5, S, ML_LATEST);
        else msg_set(P, 5, im.bytes + b, 0u);  // (a digest without a tag: the empty tag)
        KW_MSG_LIT(P, 6, S, ML_IS_REJECTED);
        return MSG_TEXT;
      }
      KW_MSG_LIT(P, 4, S, ML_REGISTRY);
      if (r.is_reg) msg_set(P, 5, im.bytes + b, r.slash0 - b);
      else KW_MSG_LIT(P, 5, S, ML_DOCKER_IO);
      if (reason == (uint32_t)KW_R_REG_NOT_ALLOWED) KW_MSG_LIT(P, 6, S, ML_NOT_ALLOWED_REG);
      else KW_MSG_LIT(P, 6, S, ML_IS_REJECTED);
      return MSG_TEXT;
    }
    case KW_R_CAP_NOT_ALLOWED: {
      if (!D.str[DG_CAPADD].off || !C.name.off || !D.capadd_off) return MSG_MISSING;
      const uint32_t cb = D.ctr_off[row], ce = D.ctr_off[row + 1];
      if (cb > ce || ce > D.nctr) return MSG_HOST;
      const uint64_t k = (uint64_t)D.capadd_off[cb] + arg;
      if (k >= D.capadd_off[ce]) return MSG_HOST;
      // the container whose add list holds entry k: the last c in [cb, ce) with capadd_off[c] <= k
      uint32_t lo = cb, hi = ce;  // (capadd_off[cb] <= k < capadd_off[ce], so cb < ce)
      while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (D.capadd_off[mid] <= k) lo = mid;
        else hi = mid;
      }
      if (!msg_entity(C.name, lo, &pn, &nn) || !msg_entity(D.str[DG_CAPADD], k, &p0, &n0)) return MSG_HOST;
      KW_MSG_LIT(P, 0, S, ML_CTR);
      msg_set(P, 1, pn, nn);
      KW_MSG_LIT(P, 2, S, ML_ADDS_CAP);
      msg_set(P, 3, p0, n0);
      KW_MSG_LIT(P, 4, S, ML_WHICH_NOT_ALLOWED);
      P->npc = 5;
      return MSG_TEXT;
    }
    case KW_R_APPARMOR: {
      if (!D.str[DG_AA].off || !C.name.off) return MSG_MISSING;
      const uint32_t cb = D.ctr_off[row], ce = D.ctr_off[row + 1];
      if (arg >= ce - cb || !msg_entity(C.name, (uint64_t)cb + arg, &pn, &nn) ||
          !msg_entity(D.str[DG_AA], (uint64_t)cb + arg, &p0, &n0))
        return MSG_HOST;
      KW_MSG_LIT(P, 0, S, ML_CTR);
      msg_set(P, 1, pn, nn);
      KW_MSG_LIT(P, 2, S, ML_USES_AA);
      msg_set(P, 3, p0, n0);
      KW_MSG_LIT(P, 4, S, ML_WHICH_NOT_ALLOWED);
      P->npc = 5;
      return MSG_TEXT;
    }
    case KW_R_LABEL_DENIED: {
      if (!D.str[DG_LK].off) return MSG_MISSING;
      const uint32_t lb = D.lbl_off[row], le = D.lbl_off[row + 1];
      if (arg >= le - lb || !msg_entity(D.str[DG_LK], (uint64_t)lb + arg, &p0, &n0)) return MSG_HOST;
      KW_MSG_LIT(P, 0, S, ML_LABEL);
      msg_set(P, 1, p0, n0);
      KW_MSG_LIT(P, 2, S, ML_IS_DENIED);
      P->npc = 3;
      return MSG_TEXT;
    }
    case KW_R_LABEL_CONSTRAINT: {
      if (!D.str[DG_LK].off || !D.str[DG_LV].off) return MSG_MISSING;
      const uint32_t lb = D.lbl_off[row], le = D.lbl_off[row + 1];
      if (arg >= le - lb || !msg_entity(D.str[DG_LK], (uint64_t)lb + arg, &p0, &n0) ||
          !msg_entity(D.str[DG_LV], (uint64_t)lb + arg, &p1, &n1))
        return MSG_HOST;
      const uint32_t e = msg_find_constraint(S, pc, p0, n0);
      if (e == 0xffffffffu) return MSG_HOST;
      KW_MSG_LIT(P, 0, S, ML_LABEL);
      msg_set(P, 1, p0, n0);
      KW_MSG_LIT(P, 2, S, ML_VALUE);
      msg_set(P, 3, p1, n1);
      KW_MSG_LIT(P, 4, S, ML_CONSTRAINT);
      msg_set_span(P, 5, S, S.cons[e].re);
      KW_MSG_LIT(P, 6, S, ML_QUOTE);
      P->npc = 7;
      return MSG_TEXT;
    }
    case KW_R_LABEL_MANDATORY:
      if (arg >= pc.nmand) return MSG_HOST;
      KW_MSG_LIT(P, 0, S, ML_MANDATORY);
      msg_set_span(P, 1, S, S.mand[pc.mand_at + arg]);
      KW_MSG_LIT(P, 2, S, ML_IS_MISSING);
      P->npc = 3;
      return MSG_TEXT;
    case KW_R_GROUP:
      msg_set_span(P, 0, S, pc.message);
      P->npc = 1;
      return MSG_TEXT;
    case KW_R_INIT_ERROR:
      msg_set_span(P, 0, S, pc.init);
      P->npc = 1;
      return MSG_TEXT;
    default: return MSG_TEXT;  // reason 0 and the reasons no product word has: the empty message
  }
}

// ---- windows -------------------------------------------------------------------------------------
// A window is kw bytes of the output, [wb, wb + kw), wb a multiple of 16: the write kernel fills it
// in LDS and stores it with aligned 16-byte stores.
constexpr uint32_t kMsgMinWindow = 256, kMsgMaxWindow = 32768, kMsgWaveItems = 64;
KW_HD inline uint32_t msg_window_bytes(int64_t asked) {
  if (asked < (int64_t)kMsgMinWindow) return kMsgMinWindow;
  if (asked > (int64_t)kMsgMaxWindow) return kMsgMaxWindow;
  return (uint32_t)asked & ~15u;
}

// The part of the message [mb, mb + ml) inside the window [wb, wb + wl): *skip bytes of the message
// come before it, *at is its place in the window, *n its length (0: none of it).
KW_HD inline void msg_clip(uint64_t mb, uint32_t ml, uint64_t wb, uint32_t wl, uint32_t* skip, uint32_t* at, uint32_t* n) {
  const uint64_t me = mb + ml, we = wb + wl;
  const uint64_t lo = mb > wb ? mb : wb, hi = me < we ? me : we;
  if (hi <= lo) {
    *skip = *at = *n = 0;
    return;
  }
  *skip = (uint32_t)(lo - mb);
  *at = (uint32_t)(lo - wb);
  *n = (uint32_t)(hi - lo);
}
// The windows the message [mb, mb + ml) touches when the walk starts at w0 (a multiple of 16) in
// windows of wl bytes; 0 for the empty message.
KW_HD inline uint64_t msg_windows_of(uint64_t mb, uint32_t ml, uint64_t w0, uint32_t wl) {
  if (ml == 0) return 0;
  return (mb + ml - 1u - w0) / wl - (mb - w0) / wl + 1u;
}
// The byte range [lo, hi) of a window as the store loop cuts it: single bytes in [lo, *body), 16-byte
// chunks at multiples of 16 in [*body, *tail), single bytes in [*tail, hi).
KW_HD inline void msg_chunks(uint64_t lo, uint64_t hi, uint64_t* body, uint64_t* tail) {
  uint64_t b = (lo + 15u) & ~(uint64_t)15u, t = hi & ~(uint64_t)15u;
  if (b > hi) b = hi;
  if (t < b) t = b;
  *body = b;
  *tail = t;
}

// Copies bytes [skip, skip + n) of the plan's message to dst (the window's memory, at the place
// msg_clip gave): single bytes up to a 4-byte boundary of dst, whole dwords after it (from a dword
// load when the source is aligned too), single bytes at the end. dst4: dst & 3.
KW_HD inline void msg_copy_window(const MsgPlan& P, uint32_t skip, uint32_t n, uint8_t* dst) {
  uint32_t at = 0;  // the piece's place in the message
  // (unrolled over the plan's eight places: every index is a constant, so the plan stays in registers)
  KW_UNROLL
  for (uint32_t k = 0; k < kMsgMaxPieces; ++k) {
    if (k >= P.npc || !n) continue;
    const uint32_t pn = P.pc[k].n;
    if (skip >= at + pn) {
      at += pn;
      continue;
    }
    const uint32_t from = skip > at ? skip - at : 0u;
    uint32_t m = pn - from;
    if (m > n) m = n;
    const uint8_t* s = P.pc[k].p + from;
    uint32_t i = 0;
    while (i < m && (((uintptr_t)(dst + i)) & 3u)) {
      dst[i] = s[i];
      ++i;
    }
    if ((((uintptr_t)(s + i)) & 3u) == 0u) {
      for (; i + 4u <= m; i += 4u) *(uint32_t*)(dst + i) = *(const uint32_t*)(s + i);
    } else {
      for (; i + 4u <= m; i += 4u)
        *(uint32_t*)(dst + i) = (uint32_t)s[i] | ((uint32_t)s[i + 1] << 8) | ((uint32_t)s[i + 2] << 16) | ((uint32_t)s[i + 3] << 24);
    }
    for (; i < m; ++i) dst[i] = s[i];
    dst += m;
    skip += m;
    n -= m;
    at += pn;
  }
}

// ---- lengths and offsets ---------------------------------------------------------------------------
// off[i] = base + the lengths before i, off[n] the total: u64, for the text of a call passes 2^32.
inline uint64_t msg_offsets(const uint32_t* len, size_t n, uint64_t base, uint64_t* off) {
  uint64_t at = base;
  for (size_t i = 0; i < n; ++i) {
    off[i] = at;
    at += len[i];
  }
  off[n] = at;
  return at;
}

}  // namespace kw
