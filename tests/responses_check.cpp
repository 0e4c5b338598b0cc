// responses_check — the AdmissionResponse bodies of chosen pairs (include/kwgpu.h kw_batch_responses,
// policy-server_amd/csrc/responses.hpp) on the host, no GPU and no Python in the process
// (tests/test_responses.py builds it with -fsanitize=address,undefined and runs it). Header only: the
// escaped length and the escaped sub-range writer against a plain restatement of json_escape
// (json.cpp) for every byte value, at every (skip, n) of short strings and into every alignment of an
// exact-size destination (a byte outside the range is the sanitizer's to catch); whole responses of
// every form against strings put together here; a response cut at every byte, so every escape is cut
// by a window's edge at each of its positions, and walked in windows the way the kernel walks them;
// the part counts of cause masks 0, 1 and 0x7fff.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "responses.hpp"

static int failures = 0, cases = 0;
#define CHECK(c, ...)                              \
  do {                                             \
    ++cases;                                       \
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

// json_escape of json.cpp without the quotes, restated plainly.
static std::string plain_escape(const std::string& s) {
  static const char* hexd = "0123456789abcdef";
  std::string o;
  for (unsigned char c : s) {
    switch (c) {
      case '"': o += "\\\""; break;
      case '\\': o += "\\\\"; break;
      case '\n': o += "\\n"; break;
      case '\r': o += "\\r"; break;
      case '\t': o += "\\t"; break;
      case '\b': o += "\\b"; break;
      case '\f': o += "\\f"; break;
      default:
        if (c < 0x20) {
          o += "\\u00";
          o += hexd[c >> 4];
          o += hexd[c & 15];
        } else {
          o += (char)c;
        }
    }
  }
  return o;
}

// Bytes [skip, skip + n) of the escaped form of s, written into an exact-size block at alignment a.
static std::string sub_range(const std::string& s, uint32_t skip, uint32_t n, uint32_t a) {
  std::vector<uint8_t> src(s.begin(), s.end());  // (exact size: a read past the string is caught)
  std::vector<uint8_t> block(a + n);
  rsp_esc_write(src.data(), (uint32_t)src.size(), skip, n, block.data() + a);
  return std::string((const char*)block.data() + a, n);
}

static void check_escape() {
  for (uint32_t c = 0; c < 256; ++c) {
    const std::string s(1, (char)c), want = plain_escape(s);
    CHECK(rsp_esc_byte_len((uint8_t)c) == want.size(), "the length of byte %u", c);
    CHECK(rsp_esc_len((const uint8_t*)s.data(), 1) == want.size(), "the span length of byte %u", c);
    CHECK(rsp_escaped(s) == want, "byte %u", c);
    for (uint32_t skip = 0; skip <= want.size(); ++skip)
      for (uint32_t n = 0; skip + n <= want.size(); ++n)
        CHECK(sub_range(s, skip, n, skip & 3u) == want.substr(skip, n), "byte %u at (%u, %u)", c, skip, n);
  }
  CHECK(rsp_esc_len(nullptr, 0) == 0 && rsp_escaped("") == "", "the empty string");
  const char pool[] = {'a', '"', '\\', '\n', '\r', '\t', '\b', '\f', 0x01, 0x1f, 0x00, (char)0xc3, (char)0xa9, (char)0xff, ' ', 0x7f};
  for (int t = 0; t < 300; ++t) {
    std::string s;
    for (uint64_t k = rnd() % 6; k; --k) s += pool[rnd() % sizeof(pool)];
    const std::string want = plain_escape(s);
    CHECK(rsp_esc_len((const uint8_t*)s.data(), (uint32_t)s.size()) == want.size(), "the length of string %d", t);
    for (uint32_t skip = 0; skip <= want.size(); ++skip)
      for (uint32_t n = 0; skip + n <= want.size(); ++n)
        for (uint32_t a = 0; a < 8; ++a)
          CHECK(sub_range(s, skip, n, a) == want.substr(skip, n), "string %d at (%u, %u) alignment %u", t, skip, n, a);
  }
}

// One row with one container under a 15-member group (column 0, members in columns 1..15), a plain
// policy (16) and a group without members (17).
struct Fixture {
  std::string uid = "u\"\x01\\\t\xc3\xa9", ns = "n\"s\x02\\", valid = "o\"nly\x03";
  std::vector<uint32_t> uid_off, ns_off, ctr_off{0, 1}, lbl_off{0, 0}, capadd_off{0, 0};
  std::vector<uint8_t> uid_bytes, ns_bytes;
  std::vector<uint64_t> table;
  std::vector<uint32_t> words;
  RspCtx X;
  static constexpr uint32_t kCols = 18;
  Fixture() {
    uid_off = {0, (uint32_t)uid.size()};
    ns_off = {0, (uint32_t)ns.size()};
    uid_bytes.assign(uid.begin(), uid.end());
    ns_bytes.assign(ns.begin(), ns.end());
    std::vector<RspColSource> cols(kCols);
    for (uint32_t c = 0; c < kCols; ++c) {
      cols[c].id = "id\"" + std::to_string(c);
      cols[c].name = "na\\me" + std::to_string(c);
      cols[c].m.ns = valid;
      cols[c].m.message = "group \"message\"\x04";
      cols[c].m.init = "init \"error\"\n";
    }
    cols[0].is_group = true;
    for (uint32_t s = 0; s < 15; ++s) cols[0].members.push_back(1 + s);
    cols[17].is_group = true;
    table = rsp_build_table(cols);
    words.assign(kCols, 0);
    memset(&X, 0, sizeof(X));
    X.C.c.rows = 1;
    X.C.c.nctr = 1;
    X.C.c.ctr_off = ctr_off.data();
    X.C.c.lbl_off = lbl_off.data();
    X.C.c.capadd_off = capadd_off.data();
    X.C.c.str[DG_NS] = DigestStr{ns_off.data(), ns_bytes.data(), 1};
    X.uid = DigestStr{uid_off.data(), uid_bytes.data(), 1};
    X.S = rsp_settings((const uint8_t*)table.data());
    X.words = words.data();
    X.npol = kCols;
  }
  std::string ns_message() const {
    return "namespace '" + plain_escape(ns) + "' is not accepted: only '" + plain_escape(valid) + "' is allowed";
  }
};

// The whole response of column col, "<host>" or "<missing>"; rendered into an exact-size block.
static std::string render(const Fixture& F, uint32_t col, uint32_t* nparts = nullptr, uint32_t* nesc = nullptr) {
  const uint32_t w = F.words[col];
  RspItem it;
  if (rsp_item(F.X.S, col, w, &it) != RSP_TEXT) return "<host>";
  uint32_t len = 0, e = 0;
  const uint32_t st = rsp_measure(F.X, 0, col, w, it, &len, &e);
  if (st == RSP_HOST) return "<host>";
  if (st == RSP_MISSING) return "<missing>";
  if (nparts) *nparts = it.nparts;
  if (nesc) *nesc = e;
  std::vector<uint8_t> out(len);
  rsp_render_window(F.X, 0, col, w, it, 0, len, out.data());
  return std::string(out.begin(), out.end());
}

constexpr uint32_t kVanilla = (uint32_t)KW_FST_VANILLA << KW_F_STATUS_SHIFT;
static uint32_t word(uint32_t reason, uint32_t arg, uint32_t flags) { return (reason << 8) | (arg << 16) | flags; }

static void check_forms() {
  Fixture F;
  const std::string U = "{\"uid\":\"" + plain_escape(F.uid) + "\"";
  uint32_t np = 0, ne = 0;
  F.words[16] = KW_BYPASS;
  CHECK(render(F, 16, &np) == U + ",\"allowed\":true}" && np == 1, "bypass");
  F.words[16] = KW_F_ALLOWED | KW_V_ALLOWED;
  CHECK(render(F, 16) == U + ",\"allowed\":true}", "allowed");
  F.words[16] = 0;
  CHECK(render(F, 16) == U + ",\"allowed\":false}", "rejected without a status");
  F.words[16] = word(KW_R_INIT_ERROR, 0, (uint32_t)KW_FST_INIT_ERROR << KW_F_STATUS_SHIFT);
  CHECK(render(F, 16) == U + ",\"allowed\":false,\"status\":{\"message\":\"init \\\"error\\\"\\n\",\"code\":500}}", "an initialisation error");
  F.words[16] = word(0, 0, (uint32_t)KW_FST_MUTATION_REFUSED << KW_F_STATUS_SHIFT);
  CHECK(render(F, 16) == U + ",\"allowed\":false,\"status\":{\"message\":\"Request rejected by policy id\\\"16. The policy attempted to mutate "
                             "the request, but it is currently configured to not allow mutations.\"}}", "a refused mutation");
  F.words[16] = word(KW_R_NAMESPACE, 0, kVanilla);
  CHECK(render(F, 16, &np, &ne) == U + ",\"allowed\":false,\"status\":{\"message\":\"" + F.ns_message() + "\"}}" && np == 3 && ne == 2,
        "a message (the uid and the namespace grow by escaping)");
  F.words[16] = word(KW_R_PRIVILEGED, 0, kVanilla | KW_F_ALLOWED);
  CHECK(render(F, 16) == U + ",\"allowed\":true,\"status\":{\"message\":\"Privileged container is not allowed\"}}", "a finding let through");
  F.words[16] = word(0, 0, kVanilla);
  CHECK(render(F, 16) == U + ",\"allowed\":false,\"status\":{\"message\":\"\"}}", "the empty message");
  // the host's
  F.words[16] = word(KW_R_NAMESPACE, 0, kVanilla | KW_F_PATCH);
  CHECK(render(F, 16) == "<host>", "a patch");
  F.words[16] = word(KW_R_GROUP_EXPR, 0, kVanilla);
  CHECK(render(F, 16) == "<host>", "reason 14");
  F.words[16] = word(KW_R_PRIVILEGED, KW_ARG_WIDE, kVanilla);
  CHECK(render(F, 16) == "<host>", "a wide argument");
  F.words[16] = word(KW_R_REG_REJECTED, 0, kVanilla);
  CHECK(render(F, 16) == "<missing>", "a column that is not there");
  F.words[16] = word(KW_R_LABEL_DENIED, 3, kVanilla);
  F.X.C.c.str[DG_LK] = F.X.C.c.str[DG_NS];
  CHECK(render(F, 16) == "<host>", "an argument the request does not hold");
  // groups: the part counts of masks 0, 1 and 0x7fff
  CHECK(rsp_nparts(0) == 3 && rsp_nparts(1) == 5 && rsp_nparts(0x7fff) == 33, "the part counts");
  for (uint32_t s = 0; s < 15; ++s) CHECK(rsp_nth_bit(0x7fff, s) == s && rsp_nth_bit(1u << s, 0) == s, "bit %u", s);
  CHECK(rsp_nth_bit(0x5050, 2) == 12 && rsp_nth_bit(0x5050, 3) == 14, "the set bits of a sparse mask");
  const std::string G = U + ",\"allowed\":false,\"status\":{\"message\":\"group \\\"message\\\"\\u0004\",\"details\":{\"causes\":[";
  for (uint32_t s = 0; s < 15; ++s) F.words[1 + s] = word(KW_R_NAMESPACE, 0, kVanilla);
  F.words[3] = KW_V_ALLOWED | KW_V_MUTATED;  // a mutated member
  F.words[0] = word(KW_R_GROUP, 0, kVanilla);
  CHECK(render(F, 0, &np) == G + "]}}}" && np == 3, "no cause");
  F.words[0] = word(KW_R_GROUP, 1, kVanilla);
  CHECK(render(F, 0, &np) == G + "{\"field\":\"spec.policies.na\\\\me1\",\"message\":\"" + F.ns_message() + "\"}]}}}" && np == 5, "one cause");
  F.words[0] = word(KW_R_GROUP, 0x7fff, kVanilla);
  std::string all = G;
  for (uint32_t s = 0; s < 15; ++s)
    all += std::string(s ? "," : "") + "{\"field\":\"spec.policies.na\\\\me" + std::to_string(1 + s) + "\",\"message\":\"" +
           (s == 2 ? std::string("mutation is not allowed inside of policy group") : F.ns_message()) + "\"}";
  CHECK(render(F, 0, &np) == all + "]}}}" && np == 33, "fifteen causes");
  F.words[0] = word(KW_R_GROUP, 0x4004, kVanilla);
  CHECK(render(F, 0, &np) == G + "{\"field\":\"spec.policies.na\\\\me3\",\"message\":\"mutation is not allowed inside of policy group\"},"
                                 "{\"field\":\"spec.policies.na\\\\me15\",\"message\":\"" + F.ns_message() + "\"}]}}}" && np == 7,
        "two causes of a sparse mask");
  F.words[0] = word(KW_R_GROUP, KW_ARG_WIDE, kVanilla);
  CHECK(render(F, 0) == "<host>", "wide causes");
  F.words[0] = word(KW_R_GROUP, 2, kVanilla);
  F.words[2] = word(KW_R_GROUP_EXPR, 0, kVanilla);
  CHECK(render(F, 0) == "<host>", "a cause the host renders");
  F.words[2] = word(KW_R_APPARMOR, KW_ARG_WIDE, kVanilla);
  CHECK(render(F, 0) == "<host>", "a cause with a wide argument");
  F.words[17] = word(KW_R_GROUP, 5, kVanilla);
  CHECK(render(F, 17, &np) == G + "]}}}" && np == 3, "causes that are no members are dropped");
  // a group with a member that is no column, an unregistered policy, a broken member
  std::vector<RspColSource> cols(2);
  cols[0].is_group = true;
  cols[0].members = {1, kRspAbsent};
  cols[1].registered = false;
  std::vector<uint64_t> t2 = rsp_build_table(cols);
  const RspSettings S2 = rsp_settings((const uint8_t*)t2.data());
  RspItem it;
  CHECK(rsp_item(S2, 0, word(KW_R_GROUP, 1, kVanilla), &it) == RSP_HOST, "a member that is no column");
  CHECK(rsp_item(S2, 0, word(KW_R_NAMESPACE, 0, kVanilla), &it) == RSP_TEXT, "its other words render");
  CHECK(rsp_item(S2, 1, KW_BYPASS, &it) == RSP_HOST && rsp_item(S2, 1, 0, &it) == RSP_TEXT, "an unregistered policy on the bypass path");
  cols[0].broken = true;
  t2 = rsp_build_table(cols);
  const RspSettings S3 = rsp_settings((const uint8_t*)t2.data());
  CHECK(rsp_item(S3, 0, 0, &it) == RSP_HOST && rsp_item(S3, 0, KW_BYPASS, &it) == RSP_TEXT, "a broken member");
}

// A response cut at every byte (every escape at each of its positions), and walked in windows.
static void check_windows() {
  Fixture F;
  for (uint32_t s = 0; s < 15; ++s) F.words[1 + s] = word(KW_R_NAMESPACE, 0, kVanilla);
  F.words[0] = word(KW_R_GROUP, 0x7fff, kVanilla);
  F.words[16] = word(KW_R_NAMESPACE, 0, kVanilla);
  for (uint32_t col : {16u, 0u}) {
    const std::string whole = render(F, col);
    const uint32_t len = (uint32_t)whole.size(), w = F.words[col];
    RspItem it;
    CHECK(rsp_item(F.X.S, col, w, &it) == RSP_TEXT && len > 100, "column %u renders", col);
    for (uint32_t cut = 0; cut <= len; ++cut) {
      std::vector<uint8_t> a(cut), b(len - cut);
      rsp_render_window(F.X, 0, col, w, it, 0, cut, a.data());
      rsp_render_window(F.X, 0, col, w, it, cut, len - cut, b.data());
      CHECK(std::string(a.begin(), a.end()) + std::string(b.begin(), b.end()) == whole, "column %u cut at %u", col, cut);
    }
    // the kernel's walk: the response at byte mb of the output, windows of wl bytes from a multiple of 16
    for (uint32_t wl : {16u, 48u, 256u, 4096u})
      for (uint64_t mb : {(uint64_t)0, (uint64_t)1, (uint64_t)15, (uint64_t)17, ((uint64_t)1 << 32) - 3}) {
        const uint64_t w0 = mb & ~(uint64_t)15u;
        std::string got;
        for (uint64_t wb = w0; wb < mb + len; wb += wl) {
          std::vector<uint8_t> lds(wl, 0xEE);
          uint32_t skip, at, n;
          msg_clip(mb, len, wb, wl, &skip, &at, &n);
          if (n) rsp_render_window(F.X, 0, col, w, it, skip, n, lds.data() + at);
          got.append((const char*)lds.data() + at, n);
          for (uint32_t i = 0; i < wl; ++i)
            if ((i < at || i >= at + n) && lds[i] != 0xEE) CHECK(false, "a byte outside the clip at %u", i);
        }
        CHECK(got == whole, "column %u from byte %llu in windows of %u", col, (unsigned long long)mb, wl);
      }
  }
}

int main() {
  check_escape();
  check_forms();
  check_windows();
  printf("responses_check: cases %d, failures %d\n", cases, failures);
  return failures ? 1 : 0;
}
