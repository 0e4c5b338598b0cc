// responses.hpp — the pure arithmetic of the AdmissionResponse bodies of chosen pairs (include/kwgpu.h
// kw_batch_responses): the JSON format_response (service.cpp) writes for one pair of a pass, cut into
// parts, each part a bounded plan of pieces. A piece is a span of bytes with its escaped length: a
// literal of the envelope, a string of the settings table (escaped once on the host, copied as it
// stands) or a string of the request (the uid, and whatever message_pieces quotes), escaped on the
// fly as json_escape (json.cpp) does. The message of the word and of every cause is message_pieces'
// plan (messages.hpp) over a second settings table whose texts are pre-escaped; a piece that points
// into the table's block is copied, any other is a request string.
//
// The shape: one lane per item walks the item's parts in a loop. Part 0 is the head up to the
// status message, part 1 the message, then two parts per cause (the field, the member's message) and
// the tail: 3 + 2 x popcount(causes) parts for a status with a message, one part for the forms
// without. A part's plan is built with constant places and walked unrolled, as messages.hpp's is, so
// it stays in registers; only the part's number is a run-time value. rsp_measure sums the parts,
// rsp_render_window writes bytes [skip, skip + n) of the response, which is what a window of the
// write kernel (reports.hip responses_write_kernel) asks for: an escape may straddle its edge.
// Every function the device runs is KW_HD: the host renderer (kw_debug_responses_words how = 1)
// runs the same code over the host columns. No HIP, no batch, no settings of the process
// (tests/responses_check.cpp runs it on the host).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "messages.hpp"

namespace kw {

// ---- JSON escaping (json.cpp json_escape, without the quotes) --------------------------------------
// The escaped length of one byte: 2 for the short escapes, 6 for \u00xx, else 1.
KW_HD inline uint32_t rsp_esc_byte_len(uint8_t c) {
  if (c == (uint8_t)'"' || c == (uint8_t)'\\') return 2u;
  if (c >= 0x20u) return 1u;
  return (c == (uint8_t)'\n' || c == (uint8_t)'\r' || c == (uint8_t)'\t' || c == (uint8_t)'\b' || c == (uint8_t)'\f') ? 2u : 6u;
}
// Byte j of the escaped form of c, l = rsp_esc_byte_len(c) (arithmetic, no table: nothing a lane
// would index in scratch).
KW_HD inline uint8_t rsp_esc_byte_at(uint8_t c, uint32_t l, uint32_t j) {
  if (l == 1u) return c;
  if (j == 0u) return (uint8_t)'\\';
  if (l == 2u) {
    switch (c) {
      case '\n': return (uint8_t)'n';
      case '\r': return (uint8_t)'r';
      case '\t': return (uint8_t)'t';
      case '\b': return (uint8_t)'b';
      case '\f': return (uint8_t)'f';
      default: return c;  // '"' and '\\'
    }
  }
  if (j == 1u) return (uint8_t)'u';
  if (j < 4u) return (uint8_t)'0';
  const uint32_t nib = j == 4u ? (uint32_t)c >> 4 : (uint32_t)c & 15u;
  return (uint8_t)(nib < 10u ? '0' + nib : 'a' + (nib - 10u));
}
// The escaped length of the span (p, n).
KW_HD inline uint32_t rsp_esc_len(const uint8_t* p, uint32_t n) {
  uint32_t l = 0;
  for (uint32_t i = 0; i < n; ++i) l += rsp_esc_byte_len(p[i]);
  return l;
}
// Writes bytes [skip, skip + m) of the escaped form of (p, n) to dst; the caller keeps skip + m within
// the escaped length. An escape the range cuts is written in part.
KW_HD inline void rsp_esc_write(const uint8_t* p, uint32_t n, uint32_t skip, uint32_t m, uint8_t* dst) {
  const uint32_t end = skip + m;
  uint32_t at = 0;  // the escaped place of p[i]
  for (uint32_t i = 0; i < n && at < end; ++i) {
    const uint8_t c = p[i];
    const uint32_t l = rsp_esc_byte_len(c);
    if (at + l > skip) {
      for (uint32_t j = 0; j < l; ++j) {
        const uint32_t g = at + j;
        if (g >= skip && g < end) dst[g - skip] = rsp_esc_byte_at(c, l, j);
      }
    }
    at += l;
  }
}
// (host: the table's texts)
inline std::string rsp_escaped(const std::string& s) {
  std::string o(rsp_esc_len((const uint8_t*)s.data(), (uint32_t)s.size()), '\0');
  if (!o.empty()) rsp_esc_write((const uint8_t*)s.data(), (uint32_t)s.size(), 0, (uint32_t)o.size(), (uint8_t*)&o[0]);
  return o;
}

// ---- the literals of the envelope, each once ---------------------------------------------------------
#define KW_RSP_LITS(X)                                              \
  X(RL_OPEN, "{\"uid\":\"")                                         \
  X(RL_TRUE, "\",\"allowed\":true}")                                \
  X(RL_FALSE, "\",\"allowed\":false}")                              \
  X(RL_ST_TRUE, "\",\"allowed\":true,\"status\":{\"message\":\"")   \
  X(RL_ST_FALSE, "\",\"allowed\":false,\"status\":{\"message\":\"") \
  X(RL_CODE500, "\",\"code\":500}}")                                \
  X(RL_END, "\"}}")                                                 \
  X(RL_NO_CAUSES, "\",\"details\":{\"causes\":[]}}}")               \
  X(RL_CAUSE_FIRST, "\",\"details\":{\"causes\":[{\"field\":\"")    \
  X(RL_CAUSE_NEXT, "\"},{\"field\":\"")                             \
  X(RL_CAUSE_MSG, "\",\"message\":\"")                              \
  X(RL_CAUSES_END, "\"}]}}}")                                       \
  X(RL_MUTATION, "mutation is not allowed inside of policy group")

enum RspLit : uint32_t {
#define X(id, s) id##_AT, id##_LAST = id##_AT + sizeof(s) - 2,
  KW_RSP_LITS(X)
#undef X
  RL_BYTES
};
enum : uint32_t {
#define X(id, s) id##_LEN = sizeof(s) - 1,
  KW_RSP_LITS(X)
#undef X
};
#define X(id, s) s
constexpr char kRspLitText[] = KW_RSP_LITS(X);
#undef X
static_assert(sizeof(kRspLitText) - 1 == RL_BYTES, "the literals' places add up to the table");

// ---- the settings table of the responses ---------------------------------------------------------------
// One block: [RspHead][RspCol x ncols][u32 x members][text][pad to 8][the messages' table]. The text
// starts with kRspLitText and holds every column's mutation-refused text and cause field, escaped.
// The messages' table is msg_build_table's block over the same columns with every text that a
// message quotes escaped (the constrained keys stay raw: they are searched, never quoted), so
// message_pieces runs on it unchanged.
enum : uint32_t {
  RC_GROUP = 1u,          // a policy group
  RC_UNREGISTERED = 2u,   // the bypass path answers PolicyNotFound: the host's
  RC_BROKEN = 4u,         // a group with a member that failed to initialise: the host's
  RC_MEMBER_ABSENT = 8u   // a group with a member that is no column of the pass
};
constexpr uint32_t kRspAbsent = 0xffffffffu;
struct RspCol {
  uint32_t flags;
  MsgSpan refused;  // "Request rejected by policy <id>. The policy attempted to mutate ..."
  MsgSpan field;    // "spec.policies.<name>"
  uint32_t mem_at, nmem;  // the members' columns, settings order (kRspAbsent: no column)
};
struct RspHead {
  uint32_t ncols, nmem, text_bytes, msg_at, bytes, pad;
};
struct RspSettings {
  const RspCol* col;
  const uint32_t* mem;
  const uint8_t* text;
  const uint8_t *lo, *hi;  // the block: a piece inside it is copied as it stands
  MsgSettings M;
  uint32_t ncols;
};
KW_HD inline RspSettings rsp_settings(const uint8_t* block) {
  const RspHead* h = (const RspHead*)block;
  RspSettings S;
  S.ncols = h->ncols;
  S.col = (const RspCol*)(block + sizeof(RspHead));
  S.mem = (const uint32_t*)(S.col + h->ncols);
  S.text = (const uint8_t*)(S.mem + h->nmem);
  S.lo = block;
  S.hi = block + h->bytes;
  S.M = msg_settings(block + h->msg_at);
  return S;
}
KW_HD inline bool rsp_owns(const RspSettings& S, const uint8_t* p) { return p >= S.lo && p < S.hi; }

// What the host hands over per column (responses.cpp fills it from PolicyRec); every string raw.
struct RspColSource {
  MsgColSource m;
  std::string id, name;
  bool registered = true, is_group = false, broken = false;
  std::vector<uint32_t> members;  // the members' columns or kRspAbsent
};
inline std::vector<uint64_t> rsp_build_table(const std::vector<RspColSource>& cols) {
  std::string text(kRspLitText, RL_BYTES);
  auto put = [&](const std::string& s) {
    MsgSpan sp{(uint32_t)text.size(), (uint32_t)s.size()};
    text += s;
    return sp;
  };
  std::vector<RspCol> C;
  std::vector<uint32_t> M;
  std::vector<MsgColSource> E;
  for (const RspColSource& s : cols) {
    RspCol c{};
    c.flags = (s.is_group ? RC_GROUP : 0u) | (s.registered ? 0u : RC_UNREGISTERED) | (s.is_group && s.broken ? RC_BROKEN : 0u);
    c.refused = put(rsp_escaped("Request rejected by policy " + s.id +
                                ". The policy attempted to mutate the request, but it is currently configured to not "
                                "allow mutations."));
    c.field = put(rsp_escaped("spec.policies." + s.name));
    c.mem_at = (uint32_t)M.size();
    c.nmem = (uint32_t)s.members.size();
    for (uint32_t m : s.members) {
      if (m == kRspAbsent || m >= cols.size()) c.flags |= RC_MEMBER_ABSENT;
      M.push_back(m < cols.size() ? m : kRspAbsent);
    }
    C.push_back(c);
    MsgColSource e;
    e.family = s.m.family;
    e.ns = rsp_escaped(s.m.ns);
    e.message = rsp_escaped(s.m.message);
    e.init = rsp_escaped(s.m.init);
    for (const std::string& x : s.m.mandatory) e.mandatory.push_back(rsp_escaped(x));
    e.keys = s.m.keys;
    for (const std::string& x : s.m.regexes) e.regexes.push_back(rsp_escaped(x));
    E.push_back(std::move(e));
  }
  const std::vector<uint64_t> msg = msg_build_table(E);
  const size_t own = sizeof(RspHead) + C.size() * sizeof(RspCol) + M.size() * 4 + text.size(), msg_at = (own + 7) & ~(size_t)7;
  RspHead h{(uint32_t)C.size(), (uint32_t)M.size(), (uint32_t)text.size(), (uint32_t)msg_at, (uint32_t)(msg_at + msg.size() * 8), 0u};
  std::vector<uint64_t> block(msg_at / 8 + msg.size(), 0);
  uint8_t* p = (uint8_t*)block.data();
  memcpy(p, &h, sizeof(h));
  p += sizeof(h);
  if (!C.empty()) memcpy(p, C.data(), C.size() * sizeof(RspCol));
  p += C.size() * sizeof(RspCol);
  if (!M.empty()) memcpy(p, M.data(), M.size() * 4);
  p += M.size() * 4;
  memcpy(p, text.data(), text.size());
  memcpy((uint8_t*)block.data() + msg_at, msg.data(), msg.size() * 8);
  return block;
}

// ---- items, parts and plans ------------------------------------------------------------------------------
constexpr uint32_t kRspMaxPieces = kMsgMaxPieces;
struct RspPiece {
  const uint8_t* p;
  uint32_t n, en;  // raw and escaped length; en != n: escaped on the fly
};
struct RspPlan {
  RspPiece pc[kRspMaxPieces];
  uint32_t npc;
  uint32_t len;   // the sum of the escaped lengths
  uint32_t nesc;  // pieces with en > n
};
enum RspStatus : uint32_t { RSP_TEXT = 0, RSP_HOST = 1, RSP_MISSING = 2 };
enum RspForm : uint32_t {
  RF_SHORT,    // {"uid":U,"allowed":B}
  RF_INIT,     // ... ,"status":{"message":I,"code":500}}
  RF_REFUSED,  // ... ,"status":{"message":R}}
  RF_MESSAGE,  // ... ,"status":{"message":M}}
  RF_GROUP     // ... ,"status":{"message":M,"details":{"causes":[...]}}}
};
struct RspItem {
  uint32_t form, nparts, mask;  // mask: the causes that are members of the column
};
// What a response is cut from: the messages' columns, the uid column, the table, the pass's words
// (rows as the columns have them) for the members' words of the same row.
struct RspCtx {
  MsgCols C;
  DigestStr uid;
  RspSettings S;
  const uint32_t* words;
  uint32_t npol;
};

KW_HD inline uint32_t rsp_popcount(uint32_t v) {
  uint32_t n = 0;
  for (; v; v &= v - 1u) ++n;
  return n;
}
// The parts of a status with a message and `mask` causes.
KW_HD inline uint32_t rsp_nparts(uint32_t mask) { return 3u + 2u * rsp_popcount(mask); }
// The place of the j-th set bit of mask (j < its popcount).
KW_HD inline uint32_t rsp_nth_bit(uint32_t mask, uint32_t j) {
  for (; j; --j) mask &= mask - 1u;
  uint32_t s = 0;
  while (s < 31u && !((mask >> s) & 1u)) ++s;
  return s;
}
// A member's word whose message the device does not render (the mutated-and-allowed member has the
// fixed text and is asked first).
KW_HD inline bool rsp_member_mutated(uint32_t mv) { return (mv & KW_V_MUTATED) && (mv & KW_V_ALLOWED); }
KW_HD inline bool rsp_member_host(uint32_t mv) { return KW_ARG(mv) == KW_ARG_WIDE || KW_REASON(mv) == (uint32_t)KW_R_GROUP_EXPR; }

// The form of the response of `word` in column col (the tests of format_response in its order), or
// RSP_HOST by the rules of the header that need no string.
KW_HD inline uint32_t rsp_item(const RspSettings& S, uint32_t col, uint32_t word, RspItem* it) {
  const RspCol& c = S.col[col];
  it->form = RF_SHORT;
  it->nparts = 1;
  it->mask = 0;
  if (word & KW_BYPASS) return (c.flags & RC_UNREGISTERED) ? RSP_HOST : RSP_TEXT;
  if ((c.flags & RC_BROKEN) || (word & KW_F_PATCH)) return RSP_HOST;
  const uint32_t fst = (word & KW_F_STATUS_MASK) >> KW_F_STATUS_SHIFT;
  if (fst == (uint32_t)KW_FST_NONE) return RSP_TEXT;
  if (fst == (uint32_t)KW_FST_INIT_ERROR) {
    it->form = RF_INIT;
    return RSP_TEXT;
  }
  if (fst == (uint32_t)KW_FST_MUTATION_REFUSED) {
    it->form = RF_REFUSED;
    return RSP_TEXT;
  }
  const uint32_t reason = KW_REASON(word), arg = KW_ARG(word);
  if (reason == (uint32_t)KW_R_GROUP_EXPR) return RSP_HOST;
  if (reason != (uint32_t)KW_R_INIT_ERROR && arg == KW_ARG_WIDE) return RSP_HOST;  // the argument is in the pass's side data
  if (reason == (uint32_t)KW_R_GROUP) {
    if (c.flags & RC_MEMBER_ABSENT) return RSP_HOST;
    it->form = RF_GROUP;
    it->mask = c.nmem >= 16u ? arg : arg & ((1u << c.nmem) - 1u);
    it->nparts = rsp_nparts(it->mask);
    return RSP_TEXT;
  }
  it->form = RF_MESSAGE;
  it->nparts = 3;
  return RSP_TEXT;
}

KW_HD inline void rsp_set(RspPlan* P, uint32_t k, const uint8_t* p, uint32_t n, uint32_t en) {
  P->pc[k].p = p;
  P->pc[k].n = n;
  P->pc[k].en = en;
  P->len += en;
  if (en > n) ++P->nesc;
}
#define KW_RSP_LIT(P, k, S, id) rsp_set((P), (k), (S).text + id##_AT, id##_LEN, id##_LEN)
KW_HD inline void rsp_set_span(RspPlan* P, uint32_t k, const RspSettings& S, MsgSpan s) { rsp_set(P, k, S.text + s.at, s.n, s.n); }
// A request string, escaped on the fly.
KW_HD inline void rsp_set_esc(RspPlan* P, uint32_t k, const uint8_t* p, uint32_t n) { rsp_set(P, k, p, n, rsp_esc_len(p, n)); }
// message_pieces' plan as a part: a piece of the table is copied, any other is a request string.
KW_HD inline void rsp_from_msg(const RspSettings& S, const MsgPlan& M, RspPlan* P) {
  P->npc = M.npc;
  KW_UNROLL
  for (uint32_t k = 0; k < kMsgMaxPieces; ++k) {
    if (k >= M.npc) continue;
    const uint8_t* p = M.pc[k].p;
    const uint32_t n = M.pc[k].n;
    rsp_set(P, k, p, n, rsp_owns(S, p) ? n : rsp_esc_len(p, n));
  }
}

// Part k of the response of `word` at (row, col), `it` from rsp_item. On RSP_HOST and RSP_MISSING the
// plan is unspecified.
KW_HD inline uint32_t rsp_part(const RspCtx& X, uint64_t row, uint32_t col, uint32_t word, const RspItem& it, uint32_t k,
                               RspPlan* P) {
  const RspSettings& S = X.S;
  P->npc = 0;
  P->len = 0;
  P->nesc = 0;
  const bool allowed = (word & KW_F_ALLOWED) != 0u;
  if (k == 0u) {
    const uint8_t* up = nullptr;
    uint32_t un = 0;
    if (!X.uid.off) return RSP_MISSING;
    (void)msg_entity(X.uid, row, &up, &un);
    KW_RSP_LIT(P, 0, S, RL_OPEN);
    rsp_set_esc(P, 1, up, un);
    if (it.form == (uint32_t)RF_SHORT) {
      if ((word & KW_BYPASS) || allowed) KW_RSP_LIT(P, 2, S, RL_TRUE);
      else KW_RSP_LIT(P, 2, S, RL_FALSE);
      P->npc = 3;
      return RSP_TEXT;
    }
    if (allowed) KW_RSP_LIT(P, 2, S, RL_ST_TRUE);
    else KW_RSP_LIT(P, 2, S, RL_ST_FALSE);
    P->npc = 3;
    if (it.form == (uint32_t)RF_INIT) {
      const MsgSpan in = S.M.col[col].init;
      rsp_set(P, 3, S.M.text + in.at, in.n, in.n);
      KW_RSP_LIT(P, 4, S, RL_CODE500);
      P->npc = 5;
    } else if (it.form == (uint32_t)RF_REFUSED) {
      rsp_set_span(P, 3, S, S.col[col].refused);
      KW_RSP_LIT(P, 4, S, RL_END);
      P->npc = 5;
    }
    return RSP_TEXT;
  }
  if (k + 1u == it.nparts) {  // the tail
    if (it.form != (uint32_t)RF_GROUP) KW_RSP_LIT(P, 0, S, RL_END);
    else if (it.mask == 0u) KW_RSP_LIT(P, 0, S, RL_NO_CAUSES);
    else KW_RSP_LIT(P, 0, S, RL_CAUSES_END);
    P->npc = 1;
    return RSP_TEXT;
  }
  MsgPlan M;
  uint32_t st;
  if (k == 1u) {
    st = message_pieces(X.C, S.M, row, col, word, &M);
  } else {
    const uint32_t j = (k - 2u) >> 1;
    const RspCol& c = S.col[col];
    const uint32_t s = rsp_nth_bit(it.mask, j);
    const uint32_t mc = s < c.nmem ? S.mem[c.mem_at + s] : kRspAbsent;
    if (mc >= X.npol || mc >= S.ncols) return RSP_HOST;
    if (((k - 2u) & 1u) == 0u) {
      if (j == 0u) KW_RSP_LIT(P, 0, S, RL_CAUSE_FIRST);
      else KW_RSP_LIT(P, 0, S, RL_CAUSE_NEXT);
      rsp_set_span(P, 1, S, S.col[mc].field);
      KW_RSP_LIT(P, 2, S, RL_CAUSE_MSG);
      P->npc = 3;
      return RSP_TEXT;
    }
    const uint32_t mv = X.words[row * X.npol + mc];
    if (rsp_member_mutated(mv)) {
      KW_RSP_LIT(P, 0, S, RL_MUTATION);
      P->npc = 1;
      return RSP_TEXT;
    }
    if (rsp_member_host(mv)) return RSP_HOST;
    st = message_pieces(X.C, S.M, row, mc, mv, &M);
  }
  if (st == (uint32_t)MSG_HOST) return RSP_HOST;
  if (st == (uint32_t)MSG_MISSING) return RSP_MISSING;
  rsp_from_msg(S, M, P);
  return RSP_TEXT;
}

// The length of the whole response (the sum of its parts) and its pieces that grew by escaping;
// RSP_HOST / RSP_MISSING as soon as a part says so (*len is then 0).
KW_HD inline uint32_t rsp_measure(const RspCtx& X, uint64_t row, uint32_t col, uint32_t word, const RspItem& it, uint32_t* len,
                                  uint32_t* nesc) {
  uint32_t l = 0, e = 0;
  *len = 0;
  *nesc = 0;
  RspPlan P;
  for (uint32_t k = 0; k < it.nparts; ++k) {
    const uint32_t st = rsp_part(X, row, col, word, it, k, &P);
    if (st != (uint32_t)RSP_TEXT) return st;
    l += P.len;
    e += P.nesc;
  }
  *len = l;
  *nesc = e;
  return RSP_TEXT;
}

// The dword copy of msg_copy_window for one span: single bytes up to a 4-byte boundary of dst, whole
// dwords after it, single bytes at the end.
KW_HD inline void rsp_copy_raw(const uint8_t* s, uint32_t m, uint8_t* dst) {
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
}

// Copies bytes [skip, skip + n) of the part's text to dst (walked unrolled over the plan's places).
KW_HD inline void rsp_copy_window(const RspPlan& P, uint32_t skip, uint32_t n, uint8_t* dst) {
  uint32_t at = 0;
  KW_UNROLL
  for (uint32_t k = 0; k < kRspMaxPieces; ++k) {
    if (k >= P.npc || !n) continue;
    const uint32_t pn = P.pc[k].en;
    if (skip >= at + pn) {
      at += pn;
      continue;
    }
    const uint32_t from = skip > at ? skip - at : 0u;
    uint32_t m = pn - from;
    if (m > n) m = n;
    if (pn == P.pc[k].n) rsp_copy_raw(P.pc[k].p + from, m, dst);
    else rsp_esc_write(P.pc[k].p, P.pc[k].n, from, m, dst);
    dst += m;
    skip += m;
    n -= m;
    at += pn;
  }
}

// Writes bytes [skip, skip + n) of the response to dst; the caller keeps skip + n within the length
// rsp_measure gave. A part that lies before skip costs its plan, one past the range is not built.
KW_HD inline void rsp_render_window(const RspCtx& X, uint64_t row, uint32_t col, uint32_t word, const RspItem& it, uint32_t skip,
                                    uint32_t n, uint8_t* dst) {
  uint32_t at = 0;
  RspPlan P;
  for (uint32_t k = 0; k < it.nparts && n; ++k) {
    if (rsp_part(X, row, col, word, it, k, &P) != (uint32_t)RSP_TEXT) return;
    const uint32_t pl = P.len;
    if (skip < at + pl) {
      const uint32_t from = skip > at ? skip - at : 0u;
      uint32_t m = pl - from;
      if (m > n) m = n;
      rsp_copy_window(P, from, m, dst);
      dst += m;
      skip += m;
      n -= m;
    }
    at += pl;
  }
}

}  // namespace kw
