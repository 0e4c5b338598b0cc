// patches_check — the JSONPatch of accepted mutations from columns (include/kwgpu.h kw_batch_patches,
// policy-server_amd/csrc/patches.hpp) on the host, no GPU and no Python in the process
// (tests/test_patches.py builds it with -fsanitize=address,undefined and runs it). Header only, over
// hand-built columns and settings: the ops of every (row, column) against a plain restatement of
// capabilities_patch over the same columns written here with std::string; the response against the
// envelope around a plain base64 encoder; every (skip, n) of the texts of up to 96 bytes
// and every skip with a // set of lengths of the long ones into exact-size destinations and exact-size raw buffers (a byte
// outside is the sanitizer's to catch); windows of every length from 1 to 40 and of 256 bytes (past the
// twelfth row: 1 to 5, 16 and 256) concatenated to the whole text; the statuses of patch_item.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "patches.hpp"

static int failures = 0, cases = 0;
#define CHECK(c, ...)                                        \
  do {                                                       \
    ++cases;                                                 \
    if (!(c)) {                                              \
      if (++failures <= 20) {                                \
        fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);                        \
        fprintf(stderr, "\n");                               \
      }                                                      \
    }                                                        \
  } while (0)

using namespace kw;

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { return rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17, rng_state; }

struct HandCol {  // a string column with exact-size arrays
  std::vector<uint32_t> off{0};
  std::vector<uint8_t> bytes;
  void push(const std::string& s) {
    bytes.insert(bytes.end(), s.begin(), s.end());
    off.push_back((uint32_t)bytes.size());
  }
  std::string at(uint32_t i) const { return std::string((const char*)bytes.data() + off[i], off[i + 1] - off[i]); }
  DigestStr view() const { return DigestStr{off.data(), bytes.data(), off.size() - 1}; }
};
struct Hand {
  std::vector<uint32_t> ctr_off{0}, capadd_off{0}, capdrop_off{0}, place;
  std::vector<uint8_t> flags, pointer;
  HandCol add, drop, uid;
  PatchCols cols() const {
    PatchCols C{};
    C.rows = pointer.size();
    C.nctr = flags.size();
    C.ctr_off = ctr_off.data();
    C.capadd_off = capadd_off.data();
    C.capdrop_off = capdrop_off.data();
    C.ctr_flags = flags.data();
    C.add = add.view();
    C.drop = drop.view();
    C.uid = uid.view();
    C.ctr_place = place.data();
    C.req_place = pointer.data();
    return C;
  }
};

static std::string plain_quote(const std::string& s) { return "\"" + rsp_escaped(s) + "\""; }
static std::string plain_list(const std::vector<std::string>& l) {
  std::string o = "[";
  for (size_t i = 0; i < l.size(); ++i) o += (i ? "," : "") + plain_quote(l[i]);
  return o + "]";
}
static std::string plain_base64(const std::string& in) {
  static const char* T = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  std::string o;
  size_t i = 0;
  for (; i + 2 < in.size(); i += 3) {
    const uint32_t x = ((uint8_t)in[i] << 16) | ((uint8_t)in[i + 1] << 8) | (uint8_t)in[i + 2];
    o += T[x >> 18], o += T[(x >> 12) & 63], o += T[(x >> 6) & 63], o += T[x & 63];
  }
  if (i + 1 == in.size()) {
    const uint32_t x = (uint8_t)in[i] << 16;
    o += T[x >> 18], o += T[(x >> 12) & 63], o += "==";
  } else if (i + 2 == in.size()) {
    const uint32_t x = ((uint8_t)in[i] << 16) | ((uint8_t)in[i + 1] << 8);
    o += T[x >> 18], o += T[(x >> 12) & 63], o += T[(x >> 6) & 63], o += '=';
  }
  return o;
}
static std::vector<std::string> uniq(const std::vector<std::string>& l) {
  std::vector<std::string> o;
  for (const auto& x : l) {
    bool dup = false;
    for (const auto& y : o) dup = dup || x == y;
    if (!dup) o.push_back(x);
  }
  return o;
}
// capabilities_patch (service.cpp) over the hand columns.
static std::string plain_ops(const Hand& H, uint32_t row, const PatchColSource& P) {
  static const char* kPointer[] = {"", "", "/spec", "/spec/template/spec", "/spec/jobTemplate/spec/template/spec"};
  const std::vector<std::string> reqd = uniq(P.required_drop), defa = uniq(P.default_add);
  std::string ops = "[";
  auto op = [&](const std::string& path, const std::string& value) {
    ops += std::string(ops.size() > 1 ? "," : "") + "{\"op\":\"add\",\"path\":\"" + path + "\",\"value\":" + value + "}";
  };
  for (uint32_t c = H.ctr_off[row]; c < H.ctr_off[row + 1] && H.pointer[row] != KW_PP_NONE; ++c) {
    auto has = [&](const HandCol& col, const std::vector<uint32_t>& off, const std::string& x) {
      for (uint32_t k = off[c]; k < off[c + 1]; ++k)
        if (col.at(k) == x) return true;
      return false;
    };
    std::vector<std::string> mdrop, madd;
    if (!has(H.drop, H.capdrop_off, "ALL"))
      for (const auto& x : reqd)
        if (!has(H.drop, H.capdrop_off, x)) mdrop.push_back(x);
    for (const auto& x : defa)
      if (!has(H.add, H.capadd_off, x) && !has(H.drop, H.capdrop_off, x)) madd.push_back(x);
    if (mdrop.empty() && madd.empty()) continue;
    const uint32_t shape = KW_PS_SHAPE(H.place[c]);
    const char* ln = (H.flags[c] & KW_CTR_INIT) ? "initContainers" : (H.flags[c] & KW_CTR_EPHEMERAL) ? "ephemeralContainers" : "containers";
    const std::string base = std::string(kPointer[H.pointer[row]]) + "/" + ln + "/" + std::to_string(KW_PS_INDEX(H.place[c])) + "/securityContext";
    std::string obj = "{";
    if (!madd.empty()) obj += "\"add\":" + plain_list(madd);
    if (!mdrop.empty()) obj += std::string(madd.empty() ? "" : ",") + "\"drop\":" + plain_list(mdrop);
    obj += "}";
    if (shape == KW_PS_NO_SC) {
      op(base, "{\"capabilities\":" + obj + "}");
    } else if (shape == KW_PS_NO_CAPS) {
      op(base + "/capabilities", obj);
    } else {
      for (int is_add = 1; is_add >= 0; --is_add) {
        const auto& l = is_add ? madd : mdrop;
        if (l.empty()) continue;
        const std::string lp = base + "/capabilities/" + (is_add ? "add" : "drop");
        if (!((shape - KW_PS_CAPS) & (is_add ? KW_PS_ADD_ARRAY : KW_PS_DROP_ARRAY))) op(lp, plain_list(l));
        else
          for (const auto& x : l) op(lp + "/-", plain_quote(x));
      }
    }
  }
  return ops + "]";
}

// Bytes [skip, skip + n) of the text in `form`, into an exact-size block at alignment a, the raw
// buffer exactly patch_raw_need(n) bytes.
static std::string sub_range(const PatchCtx& X, uint32_t row, uint32_t col, uint32_t form, uint32_t ops, uint32_t skip, uint32_t n, uint32_t a) {
  std::vector<uint8_t> block(a + n, 0xee);
  if (form == KW_PATCH_OPS) {
    patch_render_window(X, row, col, skip, n, block.data() + a);
  } else {
    std::vector<uint8_t> raw(patch_raw_need(n));
    patch_response_window(X, row, col, patch_envelope(X, row), ops, skip, n, block.data() + a, raw.data());
  }
  return std::string((const char*)block.data() + a, n);
}

constexpr uint32_t kRows = 24;

int main() {
  const char* pool[] = {"ALL", "KILL", "NET_RAW", "CHOWN", "SETUID", "q\"x", "SYS_TIME", ""};
  Hand H;
  const uint32_t big_index[] = {0, 1, 9, 10, 99, 100, 12345, KW_PS_INDEX_MASK};
  for (uint32_t r = 0; r < kRows; ++r) {
    const uint32_t pod = KW_PP_POD, none = KW_PP_NONE;
    H.pointer.push_back((uint8_t)(r < 4 ? pod + r % 3 : r == 4 ? none : pod + (uint32_t)(rnd() % 3)));
    std::string uid = "u-" + std::to_string(r);
    if (r % 5 == 0) uid += "\"\\\n\x01\xc3\xa9";
    H.uid.push(r == 7 ? "" : uid);
    for (uint64_t k = r == 5 ? 0 : 1 + rnd() % 4; k; --k) {
      H.place.push_back(KW_PS_PLACE(1 + (H.place.size() % 6), big_index[rnd() % 8]));
      H.flags.push_back((uint8_t)(rnd() % 3 == 0 ? KW_CTR_INIT : rnd() % 3 == 0 ? KW_CTR_EPHEMERAL : 0) | (uint8_t)(rnd() & KW_CTR_PRIVILEGED));
      for (uint64_t j = rnd() % 4; j; --j) H.add.push(pool[rnd() % 8]);
      for (uint64_t j = rnd() % 4; j; --j) H.drop.push(pool[1 + rnd() % 7]);
      if (rnd() % 6 == 0) H.drop.push("ALL");
      H.capadd_off.push_back((uint32_t)H.add.off.size() - 1);
      H.capdrop_off.push_back((uint32_t)H.drop.off.size() - 1);
    }
    H.ctr_off.push_back((uint32_t)H.flags.size());
  }
  std::vector<PatchColSource> src(4);
  src[0].capabilities = true;
  src[0].required_drop = {"KILL", "NET_RAW", "KILL", "q\"x"};
  src[0].default_add = {"CHOWN", "SETUID", "CHOWN"};
  src[1].required_drop = {"KILL"};  // no psp-capabilities policy
  src[2].capabilities = true;
  src[2].required_drop = {"SYS_TIME"};
  src[3].capabilities = true;
  for (int k = 0; k < 70; ++k) src[3].required_drop.push_back("CAP_" + std::to_string(k));
  src[3].default_add = {"ALL", ""};
  const std::vector<uint64_t> table = patch_build_table(src);
  PatchCtx X;
  X.C = H.cols();
  X.S = patch_settings((const uint8_t*)table.data());
  CHECK(X.S.ncols == 4 && X.S.col[0].nreq == 3 && X.S.col[0].ndef == 2 && X.S.col[3].nreq == 70, "the table's lists are de-duplicated");
  const uint32_t word = KW_F_PATCH | KW_F_ALLOWED;

  uint32_t seen_mod[3] = {0, 0, 0}, long_texts = 0;
  for (uint32_t row = 0; row < kRows; ++row)
    for (uint32_t col : {0u, 2u, 3u}) {
      CHECK(patch_item(X, row, col, word, KW_PATCH_RESPONSE) == PATCH_TEXT, "row %u col %u is rendered", row, col);
      const std::string ops = plain_ops(H, row, src[col]);
      const uint32_t l = patch_measure(X, row, col);
      CHECK(l == ops.size(), "the ops length of row %u col %u: %u, want %zu", row, col, l, ops.size());
      if (l != ops.size()) continue;
      ++seen_mod[l % 3];
      const std::string resp = "{\"uid\":\"" + rsp_escaped(H.uid.at(row)) + "\",\"allowed\":true,\"patchType\":\"JSONPatch\",\"patch\":\"" +
                               plain_base64(ops) + "\"}";
      for (uint32_t form : {(uint32_t)KW_PATCH_OPS, (uint32_t)KW_PATCH_RESPONSE}) {
        const std::string& want = form == KW_PATCH_OPS ? ops : resp;
        uint32_t len = 0;
        CHECK(patch_length(X, row, col, word, form, &len) == PATCH_TEXT && len == want.size(), "the length of row %u col %u form %u", row, col, form);
        if (len != want.size()) continue;
        CHECK(sub_range(X, row, col, form, l, 0, len, 0) == want, "row %u col %u form %u: the whole text", row, col, form);
        if (col == 3 && row) continue;  // (the 70-name column's texts are long: one of them is cut)
        const bool all = len <= 96;
        long_texts += len > 256 ? 1 : 0;
        const uint32_t some[] = {1, 2, 3, 4, 5, 7, 63, 64, 65};
        for (uint32_t skip = 0; skip <= len; ++skip) {
          if (all) {
            for (uint32_t n = 0; skip + n <= len; ++n)
              CHECK(sub_range(X, row, col, form, l, skip, n, skip & 3u) == want.substr(skip, n), "row %u col %u form %u at (%u, %u)", row, col, form, skip, n);
          } else {
            for (uint32_t n : some)
              if (skip + n <= len)
                CHECK(sub_range(X, row, col, form, l, skip, n, n & 3u) == want.substr(skip, n), "row %u col %u form %u at (%u, %u)", row, col, form, skip, n);
            CHECK(sub_range(X, row, col, form, l, skip, len - skip, 1) == want.substr(skip), "row %u col %u form %u from %u", row, col, form, skip);
          }
        }
        for (uint32_t w = 1; w <= 41; ++w) {  // windows, the way the kernel walks them
          const uint32_t wl = w == 41 ? 256u : w;
          if (row >= 12 && w > 5 && w != 16 && w != 41) continue;
          std::string got;
          for (uint32_t at = 0; at < len; at += wl) got += sub_range(X, row, col, form, l, at, at + wl < len ? wl : len - at, 0);
          CHECK(got == want, "row %u col %u form %u in windows of %u", row, col, form, wl);
        }
      }
    }
  CHECK(seen_mod[0] && seen_mod[1] && seen_mod[2], "both base64 tails and the tail-free case occur (%u %u %u)", seen_mod[0], seen_mod[1], seen_mod[2]);
  CHECK(long_texts >= 10, "texts longer than a minimum window occur (%u)", long_texts);
  CHECK(patch_measure(X, 4, 0) == 2 && patch_measure(X, 5, 0) == 2, "no Pod spec and no containers give []");

  // the statuses
  CHECK(patch_item(X, 0, 0, KW_F_ALLOWED, KW_PATCH_OPS) == PATCH_HOST, "a word without KW_F_PATCH is the host's");
  CHECK(patch_item(X, 0, 1, word, KW_PATCH_OPS) == PATCH_HOST, "a column of another family is the host's");
  CHECK(patch_item(X, kRows, 0, word, KW_PATCH_OPS) == PATCH_HOST, "a row the columns do not hold is the host's");
  {
    Hand G = H;
    G.pointer[1] = KW_PP_UNKNOWN;
    G.place[G.ctr_off[2]] = KW_PS_PLACE(KW_PS_UNKNOWN, 3);
    PatchCtx Y = X;
    Y.C = G.cols();
    uint32_t len = 7;
    CHECK(patch_length(Y, 1, 0, word, KW_PATCH_OPS, &len) == PATCH_HOST && len == 0, "an unknown pointer is the host's");
    CHECK(patch_item(Y, 2, 0, word, KW_PATCH_RESPONSE) == PATCH_HOST, "an unknown shape is the host's");
    CHECK(patch_item(Y, 0, 0, word, KW_PATCH_RESPONSE) == PATCH_TEXT, "the other rows are rendered");
    Y.C.drop.off = nullptr;
    CHECK(patch_item(Y, 0, 0, word, KW_PATCH_OPS) == PATCH_MISSING, "a capability column that is not resident is missing");
    Y = X;
    Y.C.uid.off = nullptr;
    CHECK(patch_item(Y, 0, 0, word, KW_PATCH_OPS) == PATCH_TEXT && patch_item(Y, 0, 0, word, KW_PATCH_RESPONSE) == PATCH_MISSING,
          "only the response form needs the uids");
  }
  for (uint32_t v = 0; v < 64; ++v) CHECK(patch_b64_char(v) == (uint8_t)"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"[v], "base64 digit %u", v);
  for (uint32_t n = 1; n < 200; ++n)
    for (uint32_t phase = 0; phase < 4; ++phase)
      CHECK(3u * ((phase + n + 3u) / 4u - phase / 4u) <= patch_raw_need(n), "the raw bytes under %u characters at phase %u", n, phase);

  printf("patches_check: cases %d failures %d\n", cases, failures);
  return failures ? 1 : 0;
}
