// messages_check — the messages of chosen findings (include/kwgpu.h kw_batch_messages,
// policy-server_amd/csrc/messages.hpp) on the host, no GPU and no Python in the process
// (tests/test_messages.py builds it with -fsanitize=address,undefined and runs it). Header only:
// every reason's pieces against literal expected strings; the image forms against (registry, tag)
// pairs that a restatement of image_parts (service.cpp) gives too; arguments the request does not
// hold (every column but the images in exact-size blocks: an access past one is the sanitizer's to
// catch); the offset arithmetic past 2^32; the window clipping of one message and of a wave's 64,
// walked the way the kernel walks them, for window sizes from the minimum up, the lengths around a
// window and every head and tail alignment; the settings search over 1, 2 and 1000 keys, keys that
// differ only in length, and duplicates.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "messages.hpp"

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

static uint32_t word(uint32_t reason, uint32_t arg) { return (reason << 8) | (arg << 16); }

// A string column in exact-size blocks; `pad`: the zero tail the product's pools have (the image
// scan reads whole words).
struct Strings {
  std::vector<uint32_t> off{0};
  std::vector<uint8_t> bytes;
  size_t used = 0;
  void push(const std::string& s, bool pad = false) {
    bytes.resize(used);
    bytes.insert(bytes.end(), s.begin(), s.end());
    used = bytes.size();
    off.push_back((uint32_t)used);
    if (pad) bytes.resize(used + 32, 0);
  }
  DigestStr view() const { return DigestStr{off.data(), bytes.data(), off.size() - 1}; }
};

static std::string render(const MsgPlan& P) {
  std::vector<uint8_t> out(P.len + 8, 0xEE);
  msg_copy_window(P, 0, P.len, out.data() + 4);
  for (size_t i = 0; i < 4; ++i)
    if (out[i] != 0xEE || out[4 + P.len + i] != 0xEE) return "<wrote outside>";
  return std::string((const char*)out.data() + 4, P.len);
}

// image_parts of service.cpp, restated.
static void parts(std::string_view s, std::string* registry, std::string* tag) {
  size_t at = s.find('@');
  std::string_view name = at == std::string_view::npos ? s : s.substr(0, at);
  size_t slash = name.find('/'), rest_b = 0;
  bool is_reg = false;
  if (slash != std::string_view::npos) {
    std::string_view c0 = name.substr(0, slash);
    is_reg = c0.find('.') != std::string_view::npos || c0.find(':') != std::string_view::npos || c0 == "localhost";
  }
  if (is_reg) {
    *registry = std::string(name.substr(0, slash));
    rest_b = slash + 1;
  } else {
    *registry = "docker.io";
  }
  std::string_view rest = name.substr(rest_b);
  size_t colon = rest.rfind(':');
  if (colon != std::string_view::npos) *tag = std::string(rest.substr(colon + 1));
  else if (at == std::string_view::npos) *tag = "latest";
  else tag->clear();
}

// Two requests. Row 0: containers "web" (nginx) and "side" (evil.io/x:1), capabilities add lists
// {} and {NET_ADMIN, SYS_TIME}, AppArmor profiles, labels team=a b and env=prod. Row 1: no
// container, no label.
struct Doc {
  Strings ns, name, img, aa, cap, lk, lv;
  std::vector<uint32_t> ctr_off{0, 2, 2}, lbl_off{0, 2, 2}, capadd_off{0, 0, 2};
  MsgCols C{};
  std::vector<uint64_t> table;
  MsgSettings S{};
  Doc() {
    ns.push("prod");
    ns.push("");
    name.push("web");
    name.push("side");
    img.push("nginx", true);
    img.push("evil.io/x:1", true);
    aa.push("runtime/default");
    aa.push("localhost/evil");
    cap.push("NET_ADMIN");
    cap.push("SYS_TIME");
    lk.push("team");
    lk.push("env");
    lv.push("a b");
    lv.push("prod");
    C.c.rows = 2;
    C.c.nctr = 2;
    C.c.ctr_off = ctr_off.data();
    C.c.lbl_off = lbl_off.data();
    C.c.capadd_off = capadd_off.data();
    C.c.str[DG_NS] = ns.view();
    C.c.str[DG_IMG] = img.view();
    C.c.str[DG_AA] = aa.view();
    C.c.str[DG_CAPADD] = cap.view();
    C.c.str[DG_LK] = lk.view();
    C.c.str[DG_LV] = lv.view();
    C.name = name.view();
    MsgColSource p;
    p.family = 3;
    p.ns = "only";
    p.message = "the group's message";
    p.init = "settings are invalid";
    p.mandatory = {"owner", "cost-centre"};
    p.keys = {"team", "env"};
    p.regexes = {"^[a-z]+$", "^(dev|test)$"};
    table = msg_build_table({p, MsgColSource{}});
    S = msg_settings((const uint8_t*)table.data());
  }
  std::string text(uint64_t row, uint32_t col, uint32_t w, uint32_t want_status = MSG_TEXT) {
    MsgPlan P;
    const uint32_t st = message_pieces(C, S, row, col, w, &P);
    CHECK(st == want_status, "status %u of word %08x, wanted %u", st, w, want_status);
    CHECK(P.npc <= kMsgMaxPieces, "%u pieces", P.npc);
    if (st != MSG_TEXT) CHECK(P.len == 0 && P.npc == 0, "a plan beside status %u", st);
    return render(P);
  }
};

static void check_reasons() {
  Doc d;
  auto is = [&](uint32_t reason, uint32_t arg, const char* want) {
    const std::string got = d.text(0, 0, word(reason, arg));
    CHECK(got == want, "reason %u arg %u: '%s'", reason, arg, got.c_str());
  };
  is(0, 0, "");
  is(KW_R_PRIVILEGED, 1, "Privileged container is not allowed");
  is(KW_R_NAMESPACE, 0, "namespace 'prod' is not accepted: only 'only' is allowed");
  is(KW_R_REG_NOT_ALLOWED, 1, "container 'side' uses image 'evil.io/x:1': registry 'evil.io' is not in the allowed registries");
  is(KW_R_REG_NOT_ALLOWED, 0, "container 'web' uses image 'nginx': registry 'docker.io' is not in the allowed registries");
  is(KW_R_REG_REJECTED, 1, "container 'side' uses image 'evil.io/x:1': registry 'evil.io' is rejected");
  is(KW_R_TAG_REJECTED, 1, "container 'side' uses image 'evil.io/x:1': tag '1' is rejected");
  is(KW_R_TAG_REJECTED, 0, "container 'web' uses image 'nginx': tag 'latest' is rejected");
  is(KW_R_IMG_NOT_ALLOWED, 0, "container 'web' uses image 'nginx', which is not in the allowed images");
  is(KW_R_IMG_REJECTED, 1, "container 'side' uses image 'evil.io/x:1', which is rejected");
  is(KW_R_CAP_NOT_ALLOWED, 0, "container 'side' adds capability 'NET_ADMIN', which is not allowed");
  is(KW_R_CAP_NOT_ALLOWED, 1, "container 'side' adds capability 'SYS_TIME', which is not allowed");
  is(KW_R_APPARMOR, 1, "container 'side' uses AppArmor profile 'localhost/evil', which is not allowed");
  is(KW_R_LABEL_DENIED, 1, "label 'env' is denied");
  is(KW_R_LABEL_CONSTRAINT, 0, "label 'team' value 'a b' does not match the constraint '^[a-z]+$'");
  is(KW_R_LABEL_CONSTRAINT, 1, "label 'env' value 'prod' does not match the constraint '^(dev|test)$'");
  is(KW_R_LABEL_MANDATORY, 1, "mandatory label 'cost-centre' is missing");
  is(KW_R_GROUP, 5, "the group's message");
  is(KW_R_GROUP, KW_ARG_WIDE, "the group's message");  // the text does not read the causes
  is(KW_R_INIT_ERROR, 0, "settings are invalid");
  is(0xA5, 0xA5A5, "");  // the poison sentinel: a reason no product word has
  CHECK(d.text(0, 0, 0xA5A5A5A5u) == "", "the sentinel itself");
  CHECK(d.text(1, 0, word(KW_R_NAMESPACE, 0)) == "namespace '' is not accepted: only 'only' is allowed", "an empty namespace");
  CHECK(d.text(0, 1, word(KW_R_NAMESPACE, 0)) == "namespace 'prod' is not accepted: only '' is allowed", "an empty list");
  // left to the host: reason 14 and the wide arguments of reasons 1-12
  d.text(0, 0, word(KW_R_GROUP_EXPR, 0), MSG_HOST);
  for (uint32_t r = 1; r <= 12; ++r) d.text(0, 0, word(r, KW_ARG_WIDE), MSG_HOST);
  // the literal table is the concatenation the places were counted over
  CHECK(std::string(kMsgLitText + ML_LATEST_AT, ML_LATEST_LEN) == "latest", "the last fragment");
  CHECK(std::string(kMsgLitText + ML_CTR_AT, ML_CTR_LEN) == "container '", "a middle fragment");
  CHECK(ML_PRIVILEGED_AT == 0 && ML_LATEST_AT + ML_LATEST_LEN == ML_BYTES, "the table's ends");
}

static void check_images() {
  struct Case {
    const char *image, *registry, *tag;
  } cases_[] = {
      {"nginx", "docker.io", "latest"},
      {"a/b", "docker.io", "latest"},
      {"evil.io/x:1", "evil.io", "1"},
      {"localhost:5000/a/b@sha256:0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef", "localhost:5000", ""},
      {"localhost/x", "localhost", "latest"},
      {"reg:5000/x", "reg:5000", "latest"},  // a ':' in the registry only
      {"evil.io/x@sha256:0123456789abcdef", "evil.io", ""},  // a digest without a tag
      {"evil.io/x:7@sha256:0123456789abcdef", "evil.io", "7"},
      {"a:b", "docker.io", "b"},
      {"localhos/x", "docker.io", "latest"},
      {"", "docker.io", "latest"},
  };
  for (const Case& c : cases_) {
    std::string reg, tag;
    parts(c.image, &reg, &tag);
    CHECK(reg == c.registry && tag == c.tag, "image_parts('%s') = ('%s', '%s')", c.image, reg.c_str(), tag.c_str());
    for (uint32_t lead = 0; lead < 4; ++lead) {  // every alignment of the string in its pool
      Doc d;
      d.img = Strings();
      d.img.push(std::string(lead, 'x'), true);
      d.img.push(c.image, true);
      d.C.c.str[DG_IMG] = d.img.view();
      const std::string head = std::string("container 'side' uses image '") + c.image + "'";
      CHECK(d.text(0, 0, word(KW_R_REG_REJECTED, 1)) == head + ": registry '" + c.registry + "' is rejected", "registry of '%s'", c.image);
      CHECK(d.text(0, 0, word(KW_R_TAG_REJECTED, 1)) == head + ": tag '" + c.tag + "' is rejected", "tag of '%s'", c.image);
    }
  }
}

static void check_absent_arguments() {
  Doc d;
  // the container, the capability and the label past the request, in both rows
  for (uint32_t r : {1u, 3u, 4u, 5u, 6u, 7u, 9u}) {
    if (r == 1) continue;  // (its text quotes nothing)
    d.text(0, 0, word(r, 2), MSG_HOST);
    d.text(0, 0, word(r, 0xfffe), MSG_HOST);
    d.text(1, 0, word(r, 0), MSG_HOST);
  }
  d.text(0, 0, word(KW_R_CAP_NOT_ALLOWED, 2), MSG_HOST);
  d.text(0, 0, word(KW_R_CAP_NOT_ALLOWED, 0xfffe), MSG_HOST);
  d.text(1, 0, word(KW_R_CAP_NOT_ALLOWED, 0), MSG_HOST);
  for (uint32_t r : {(uint32_t)KW_R_LABEL_DENIED, (uint32_t)KW_R_LABEL_CONSTRAINT}) {
    d.text(0, 0, word(r, 2), MSG_HOST);
    d.text(0, 0, word(r, 0xfffe), MSG_HOST);
    d.text(1, 0, word(r, 0), MSG_HOST);
  }
  d.text(0, 0, word(KW_R_LABEL_MANDATORY, 2), MSG_HOST);
  d.text(0, 1, word(KW_R_LABEL_MANDATORY, 0), MSG_HOST);
  d.text(0, 1, word(KW_R_LABEL_CONSTRAINT, 0), MSG_HOST);  // a key the column's policy does not constrain
  // offsets that point past a column (a corrupt request): nothing is read past it
  d.ctr_off = {0, 2, 9};
  d.C.c.ctr_off = d.ctr_off.data();
  d.text(1, 0, word(KW_R_IMG_REJECTED, 3), MSG_HOST);
  d.text(1, 0, word(KW_R_APPARMOR, 6), MSG_HOST);
  d.text(1, 0, word(KW_R_CAP_NOT_ALLOWED, 0), MSG_HOST);
  // a column that is not there
  Doc e;
  e.C.name = DigestStr{nullptr, nullptr, 0};
  e.text(0, 0, word(KW_R_IMG_REJECTED, 0), MSG_MISSING);
  e.text(0, 0, word(KW_R_APPARMOR, 0), MSG_MISSING);
  e.text(0, 0, word(KW_R_CAP_NOT_ALLOWED, 0), MSG_MISSING);
  CHECK(e.text(0, 0, word(KW_R_LABEL_DENIED, 0)) == "label 'team' is denied", "a message that does not quote it");
  e.C.c.str[DG_LV] = DigestStr{nullptr, nullptr, 0};
  e.text(0, 0, word(KW_R_LABEL_CONSTRAINT, 0), MSG_MISSING);
}

static void check_offsets() {
  const size_t n = 5000;
  std::vector<uint32_t> len(n);
  for (size_t i = 0; i < n; ++i) len[i] = 0x00200000u + (uint32_t)(rnd() % 1000);  // 2 MiB each: 10 GB in all
  std::vector<uint64_t> off(n + 1);
  const uint64_t base = 0xfffffff0ull;
  const uint64_t end = msg_offsets(len.data(), n, base, off.data());
  uint64_t at = base;
  bool ok = true;
  for (size_t i = 0; i < n; ++i) {
    ok = ok && off[i] == at;
    at += len[i];
  }
  CHECK(ok && off[n] == at && end == at && at > (1ull << 33), "offsets past 2^32");
  CHECK(msg_offsets(len.data(), 0, 7, off.data()) == 7 && off[0] == 7, "no item");
}

// The kernel's walk over one wave's items on the host: windows of wl bytes from the aligned-down
// start of the range, each lane's clip copied into the window, then the window's part of the range
// stored in head bytes, 16-byte chunks and tail bytes. `out` holds the bytes before `rb` and after
// `re` too: nothing outside [rb, re) may change.
static void walk_wave(const std::vector<MsgPlan>& plans, const std::vector<uint64_t>& off, uint32_t wl, std::vector<uint8_t>* out,
                      uint64_t out_base, uint64_t* nwin, uint64_t* span) {
  const size_t n = plans.size();
  const uint64_t rb = off[0], re = off[n], w0 = rb & ~15ull;
  std::vector<uint8_t> lds(wl);
  *nwin = *span = 0;
  if (re <= rb) return;  // (as the kernel: 64 empty messages)
  for (size_t i = 0; i < n; ++i) *span += msg_windows_of(off[i], plans[i].len, w0, wl) > 1 ? 1 : 0;
  for (uint64_t wb = w0; wb < re; wb += wl, ++*nwin) {
    std::fill(lds.begin(), lds.end(), 0xCD);
    for (size_t i = 0; i < n; ++i) {
      uint32_t skip, at, m;
      msg_clip(off[i], plans[i].len, wb, wl, &skip, &at, &m);
      CHECK((uint64_t)at + m <= wl && (uint64_t)skip + m <= plans[i].len, "a clip outside its window or message");
      if (m) msg_copy_window(plans[i], skip, m, lds.data() + at);
    }
    const uint64_t lo = std::max(wb, rb), hi = std::min(wb + wl, re);
    uint64_t body, tail;
    msg_chunks(lo, hi, &body, &tail);
    CHECK(lo <= body && body <= tail && tail <= hi && body - lo < 16 && hi - tail < 16, "the cut of [%llu, %llu)",
          (unsigned long long)lo, (unsigned long long)hi);
    CHECK(body == tail || (body % 16 == 0 && tail % 16 == 0), "unaligned chunks");
    for (uint64_t g = lo; g < body; ++g) (*out)[g - out_base] = lds[g - wb];
    for (uint64_t g = body; g < tail; g += 16) memcpy(out->data() + (g - out_base), lds.data() + (g - wb), 16);
    for (uint64_t g = tail; g < hi; ++g) (*out)[g - out_base] = lds[g - wb];
  }
}

static void check_windows() {
  // pieces over one pool of random bytes, at every source alignment
  std::vector<uint8_t> pool(1 << 16);
  for (uint8_t& b : pool) b = (uint8_t)rnd();
  auto plan_of = [&](uint32_t len) {
    MsgPlan P;
    P.npc = 0;
    P.len = 0;
    uint32_t left = len;
    for (uint32_t k = 0; k < kMsgMaxPieces && left; ++k) {
      uint32_t m = k + 1 == kMsgMaxPieces ? left : (uint32_t)(rnd() % (left + 1));
      if (k == 2) m = 0;  // an empty piece among them
      msg_put(&P, pool.data() + rnd() % 1000, m);
      left -= m;
    }
    if (left) {  // (the last piece takes the rest)
      P.pc[P.npc - 1].n += left;
      P.len += left;
    }
    return P;
  };
  auto flat = [&](const MsgPlan& P) {
    std::string s;
    for (uint32_t k = 0; k < P.npc; ++k) s.append((const char*)P.pc[k].p, P.pc[k].n);
    return s;
  };
  for (uint32_t wl : {kMsgMinWindow, 272u, 1024u, 4096u}) {
    CHECK(msg_window_bytes(wl) == wl, "a window size that stands");
    const uint32_t lens[] = {0, 1, wl - 1, wl, wl + 1, 5 * wl + 3};
    // one message at every head alignment (the tail alignments follow from the lengths)
    for (uint32_t len : lens)
      for (uint32_t a = 0; a < 16; ++a)
        for (uint32_t extra = 0; extra < (len == wl ? 16u : 1u); ++extra) {
          const uint32_t l = len + extra;
          const MsgPlan P = plan_of(l);
          const uint64_t rb = (1ull << 32) + 4096 + a, base = rb - 64;
          std::vector<uint8_t> out(64 + l + 64, 0xEE);
          uint64_t nwin, span;
          walk_wave({P}, {rb, rb + l}, wl, &out, base, &nwin, &span);
          const std::string want = flat(P);
          CHECK(memcmp(out.data() + 64, want.data(), l) == 0, "window %u length %u alignment %u", wl, l, a);
          bool clean = true;
          for (uint32_t i = 0; i < 64; ++i) clean = clean && out[i] == 0xEE && out[64 + l + i] == 0xEE;
          CHECK(clean, "window %u length %u alignment %u wrote outside its range", wl, l, a);
          const uint64_t w0 = rb & ~15ull, want_win = l ? (rb + l - 1 - w0) / wl + 1 : 0;
          CHECK(nwin == want_win && span == (want_win > 1 ? 1u : 0u), "window %u length %u alignment %u: %llu windows", wl, l, a,
                (unsigned long long)nwin);
        }
    // a wave's 64 messages, the lengths of the list mixed with short ones
    for (uint32_t round = 0; round < 24; ++round) {
      std::vector<MsgPlan> plans;
      std::vector<uint64_t> off;
      const uint64_t rb = (3ull << 32) + round * 17 + (round % 16), base = rb - 64;
      uint64_t at = rb;
      std::string want;
      for (uint32_t i = 0; i < kMsgWaveItems; ++i) {
        const uint32_t l = rnd() % 5 == 0 ? lens[rnd() % 6] : (uint32_t)(rnd() % 130);
        plans.push_back(plan_of(l));
        off.push_back(at);
        at += l;
        want += flat(plans.back());
      }
      off.push_back(at);
      std::vector<uint8_t> out(64 + want.size() + 64, 0xEE);
      uint64_t nwin, span;
      walk_wave(plans, off, wl, &out, base, &nwin, &span);
      CHECK(memcmp(out.data() + 64, want.data(), want.size()) == 0, "window %u wave %u", wl, round);
      bool clean = true;
      for (uint32_t i = 0; i < 64; ++i) clean = clean && out[i] == 0xEE && out[64 + want.size() + i] == 0xEE;
      CHECK(clean, "window %u wave %u wrote outside its range", wl, round);
    }
  }
  CHECK(msg_window_bytes(0) == kMsgMinWindow && msg_window_bytes(1 << 30) == kMsgMaxWindow && msg_window_bytes(1000) == 992,
        "the window size's bounds");
}

static void check_settings_search() {
  auto find = [](const MsgSettings& S, uint32_t col, const std::string& k) -> std::string {
    const uint32_t e = msg_find_constraint(S, S.col[col], (const uint8_t*)k.data(), (uint32_t)k.size());
    if (e == 0xffffffffu) return "<none>";
    return std::string((const char*)S.text + S.cons[e].re.at, S.cons[e].re.n);
  };
  MsgColSource one, two, many, none;
  one.keys = {"k"};
  one.regexes = {"r-k"};
  two.keys = {"b", "a"};
  two.regexes = {"r-b", "r-a"};
  // keys that differ only in length, duplicates (the first in settings order wins), the empty key
  const char* shapes[] = {"a", "aa", "aaa", "", "ab", "b", "aa", "a", "ba"};
  for (size_t i = 0; i < sizeof(shapes) / sizeof(shapes[0]); ++i) {
    many.keys.push_back(shapes[i]);
    many.regexes.push_back("shape-" + std::to_string(i));
  }
  for (int i = 0; i < 1000; ++i) {
    many.keys.push_back("key" + std::to_string(rnd() % 700));  // (duplicates among them)
    many.regexes.push_back("re-" + std::to_string(i));
  }
  const std::vector<uint64_t> table = msg_build_table({one, two, many, none});
  const MsgSettings S = msg_settings((const uint8_t*)table.data());
  CHECK(S.ncols == 4 && S.col[2].ncons == many.keys.size() && S.col[3].ncons == 0, "the table's shape");
  CHECK(find(S, 0, "k") == "r-k" && find(S, 0, "j") == "<none>" && find(S, 0, "kk") == "<none>" && find(S, 0, "") == "<none>", "one key");
  CHECK(find(S, 1, "a") == "r-a" && find(S, 1, "b") == "r-b" && find(S, 1, "c") == "<none>" && find(S, 1, "ab") == "<none>", "two keys");
  CHECK(find(S, 3, "a") == "<none>", "no key");
  for (const std::string& k : many.keys) {
    size_t first = 0;
    while (many.keys[first] != k) ++first;  // the entry policy_message's linear walk finds
    CHECK(find(S, 2, k) == many.regexes[first], "key '%s'", k.c_str());
  }
  CHECK(find(S, 2, "aaaa") == "<none>" && find(S, 2, "key") == "<none>" && find(S, 2, "zzzzzzzzzz") == "<none>", "keys that are not there");
  for (uint32_t i = 1; i < S.col[2].ncons; ++i) {
    const MsgCons &x = S.cons[S.col[2].cons_at + i - 1], &y = S.cons[S.col[2].cons_at + i];
    CHECK(msg_key_cmp(S.text + x.key.at, x.key.n, S.text + y.key.at, y.key.n) <= 0, "the order at %u", i);
  }
}

int main() {
  check_reasons();
  check_images();
  check_absent_arguments();
  check_offsets();
  check_windows();
  check_settings_search();
  printf("messages_check: cases %d, failures %d\n", cases, failures);
  return failures ? 1 : 0;
}
