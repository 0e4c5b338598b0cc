// packed_check — the packed verdict form (include/kwgpu.h kw_packed, policy-server_amd/csrc/packed.hpp)
// on the host, no GPU and no Python in the process (tests/test_packed.py builds it with
// -fsanitize=address,undefined and runs it): verdict words of the host walk over synthetic batches
// go through kw_debug_pack_words, and kw_packed_unpack / kw_packed_word must give every word back;
// the offsets, the exception count, the padding bits and the capacity error are checked on the way.
//   usage: packed_check <repository root>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/kwgpu.h"
#include "packed.hpp"

extern "C" {
struct kws_batch;
kws_batch* kws_generate(int config, uint64_t n, uint64_t seed, uint64_t row0);
int kws_view(const kws_batch* b, kw_soa* s);
void kws_free(kws_batch* b);
}

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

struct Arrays {
  std::vector<uint64_t> planes;
  std::vector<uint32_t> off, exc, dict;
  kw_packed p;
  Arrays(uint64_t rows, uint32_t npol, size_t cap)
      : planes(kw::packed_plane_words(rows, npol), ~0ull), off(rows + 1, 0xdeadbeefu), exc(cap, 0u), dict(3 * (size_t)npol, 0u) {
    p = kw_packed{rows, npol, planes.data(), off.data(), exc.data(), cap, dict.data(), 0};
  }
};

// Every property of a packed pass over `words` (rows x npol) under env's dictionary; returns the
// exception count.
static size_t check_words(const char* what, const kw_env* env, const std::vector<int32_t>& pol, int origin,
                          const std::vector<uint32_t>& words, uint64_t rows, bool no_reason0) {
  ++cases;
  const uint32_t npol = (uint32_t)pol.size(), G = kw::packed_groups(npol);
  Arrays a(rows, npol, rows * npol);
  int rc = kw_debug_pack_words(env, pol.data(), npol, origin, words.data(), rows, &a.p);
  CHECK(rc == KW_OK, "%s: pack rc %d", what, rc);
  if (rc != KW_OK) return 0;
  // the exceptions are exactly the words their column's dictionary does not hold
  size_t absent = 0;
  for (uint64_t r = 0; r < rows; ++r)
    for (uint32_t c = 0; c < npol; ++c) {
      const uint32_t w = words[r * npol + c], *d = &a.dict[3 * c];
      absent += w != d[0] && w != d[1] && w != d[2];
    }
  CHECK(a.p.exc_count == absent, "%s: exc_count %zu, words outside the dictionary %zu", what, a.p.exc_count, absent);
  CHECK(a.off[rows] == a.p.exc_count, "%s: exc_off[rows] %u vs exc_count %zu", what, a.off[rows], a.p.exc_count);
  for (uint64_t r = 0; r < rows; ++r) CHECK(a.off[r] <= a.off[r + 1], "%s: exc_off decreases at row %llu", what, (unsigned long long)r);
  if (rows) CHECK(a.off[0] == 0, "%s: exc_off[0] %u", what, a.off[0]);
  // plane bits of columns >= npol are 0
  if (npol % 64)
    for (uint64_t r = 0; r < rows; ++r)
      for (int h = 0; h < 2; ++h)
        CHECK((a.planes[2 * (r * G + G - 1) + h] >> (npol % 64)) == 0, "%s: padding bits set in row %llu", what, (unsigned long long)r);
  std::vector<uint32_t> back(words.size(), 0x5a5a5a5au);
  rc = kw_packed_unpack(&a.p, 0, rows, back.data());
  CHECK(rc == KW_OK && back == words, "%s: unpack rc %d differs from the input", what, rc);
  if (rows > 3) {  // an inner row range
    std::vector<uint32_t> part((size_t)(rows - 3) * npol);
    rc = kw_packed_unpack(&a.p, 2, rows - 1, part.data());
    CHECK(rc == KW_OK && !memcmp(part.data(), words.data() + 2 * npol, part.size() * 4), "%s: unpack of rows [2, rows - 1)", what);
  }
  size_t bad = 0;
  for (uint64_t r = 0; r < rows; ++r)
    for (uint32_t c = 0; c < npol; ++c) {
      uint32_t w = 0;
      bad += kw_packed_word(&a.p, r, c, &w) != KW_OK || w != words[r * npol + c];
    }
  CHECK(bad == 0, "%s: word(r, c) differs on %zu pairs", what, bad);
  uint32_t w;
  CHECK(kw_packed_word(&a.p, rows, 0, &w) == KW_E_ARG && kw_packed_word(&a.p, 0, npol, &w) == KW_E_ARG, "%s: word outside the pass", what);
  if (no_reason0)
    for (size_t i = 0; i < a.p.exc_count; ++i) CHECK(KW_REASON(a.exc[i]) != 0, "%s: escaped word %08x has REASON 0", what, a.exc[i]);
  // deterministic: a second run gives the same bytes
  Arrays b(rows, npol, rows * npol);
  rc = kw_debug_pack_words(env, pol.data(), npol, origin, words.data(), rows, &b.p);
  CHECK(rc == KW_OK && a.planes == b.planes && a.off == b.off && a.dict == b.dict &&
            !memcmp(a.exc.data(), b.exc.data(), a.p.exc_count * 4), "%s: a second run differs", what);
  // capacity: exact fits, one word short is KW_E_NOSPACE with the exact need
  if (absent) {
    Arrays c(rows, npol, absent);
    CHECK(kw_debug_pack_words(env, pol.data(), npol, origin, words.data(), rows, &c.p) == KW_OK, "%s: exact capacity", what);
    Arrays s(rows, npol, absent - 1);
    rc = kw_debug_pack_words(env, pol.data(), npol, origin, words.data(), rows, &s.p);
    CHECK(rc == KW_E_NOSPACE && s.p.exc_count == absent, "%s: one word short: rc %d need %zu (want %zu)", what, rc, s.p.exc_count, absent);
  }
  return absent;
}

static kw_env* build_env(const std::string& root, const char* name) {
  const std::string path = root + "/configs/" + name + ".yml";
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return nullptr;
  std::string text;
  char tmp[65536];
  for (size_t m; (m = fread(tmp, 1, sizeof(tmp), f)) > 0;) text.append(tmp, m);
  fclose(f);
  kw_env_options o{1, "kubewarden", -1};
  kw_env* env = nullptr;
  char err[512] = "";
  if (kw_env_build_yaml(text.data(), text.size(), &o, &env, err, sizeof(err)) != KW_OK) {
    fprintf(stderr, "%s: %s\n", path.c_str(), err);
    return nullptr;
  }
  return env;
}

static bool walk(const kw_env* env, int cfg, uint64_t rows, const std::vector<int32_t>& pol, int origin, std::vector<uint32_t>* words) {
  kws_batch* sb = kws_generate(cfg, rows, 7100 + cfg, 0);
  kw_soa soa;
  kw_batch* b = nullptr;
  bool ok = sb && kws_view(sb, &soa) == 0 && kw_batch_from_soa(&soa, &b) == KW_OK;
  words->assign(rows * pol.size(), 0);
  ok = ok && kw_debug_host_walk(env, b, pol.data(), (uint32_t)pol.size(), origin, words->data()) == KW_OK;
  if (b) kw_batch_destroy(b);
  if (sb) kws_free(sb);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 2) return fprintf(stderr, "usage: packed_check <repository root>\n"), 2;
  const std::string root = argv[1];
  const uint64_t rows = 2000;
  struct Cfg {
    const char* name;
    int synth;
  } cfgs[] = {{"c4_64", 4}, {"parity", 0}, {"c3_group", 3}, {"c6_256", 6}};
  for (const Cfg& c : cfgs) {
    kw_env* env = build_env(root, c.name);
    if (!env) return fprintf(stderr, "no environment %s\n", c.name), 2;
    const int np = kw_env_policy_count(env);
    std::vector<int32_t> all(np);
    for (int i = 0; i < np; ++i) all[i] = i;
    for (int origin : {KW_ORIGIN_VALIDATE, KW_ORIGIN_AUDIT}) {
      std::vector<uint32_t> words;
      if (!walk(env, c.synth, rows, all, origin, &words)) return fprintf(stderr, "host walk %s failed\n", c.name), 2;
      const std::string what = std::string(c.name) + (origin == KW_ORIGIN_AUDIT ? " audit" : " validate");
      const size_t exc = check_words(what.c_str(), env, all, origin, words, rows, !strcmp(c.name, "c4_64"));
      printf("%s: %d columns, exceptions %.4f of the words\n", what.c_str(), np, (double)exc / (double)(rows * np));
    }
    if (!strcmp(c.name, "c6_256")) {  // column counts around the 64-column groups, as prefixes
      for (int n : {1, 4, 63, 64, 65, 128, 296}) {
        if (n > np) return fprintf(stderr, "c6_256 has %d policies, fewer than %d\n", np, n), 2;
        std::vector<int32_t> pre(all.begin(), all.begin() + n);
        std::vector<uint32_t> words;
        if (!walk(env, c.synth, 300, pre, KW_ORIGIN_VALIDATE, &words)) return fprintf(stderr, "host walk prefix %d failed\n", n), 2;
        check_words(("c6 prefix " + std::to_string(n)).c_str(), env, pre, KW_ORIGIN_VALIDATE, words, 300, false);
      }
    }
    if (!strcmp(c.name, "c4_64")) {  // hand-made arrays under C4's dictionary
      const uint32_t npol = (uint32_t)np;
      Arrays z(0, npol, 0);  // 0 rows: the dictionary alone
      ++cases;
      int rc = kw_debug_pack_words(env, all.data(), npol, KW_ORIGIN_VALIDATE, nullptr, 0, &z.p);
      CHECK(rc == KW_OK && z.p.exc_count == 0 && z.off[0] == 0, "0 rows: rc %d", rc);
      CHECK(kw_packed_unpack(&z.p, 0, 0, nullptr) == KW_OK, "0 rows: unpack");
      // row 0: every word an exception (the poison word among them); row 1: none (each dictionary
      // entry in turn); row 2: one poisoned word among coded ones
      std::vector<uint32_t> w(3 * (size_t)npol);
      for (uint32_t col = 0; col < npol; ++col) {
        w[col] = col == 5 ? 0xA5A5A5A5u : (0x00010100u + (col << 16));
        w[npol + col] = z.dict[3 * col + col % 3];
        w[2 * npol + col] = col == npol - 1 ? 0xA5A5A5A5u : z.dict[3 * col];
      }
      const size_t exc = check_words("hand-made", env, all, KW_ORIGIN_VALIDATE, w, 3, false);
      CHECK(exc == (size_t)npol + 1, "hand-made: %zu exceptions, want %u", exc, npol + 1);
      Arrays h(3, npol, 3 * (size_t)npol);
      rc = kw_debug_pack_words(env, all.data(), npol, KW_ORIGIN_VALIDATE, w.data(), 3, &h.p);
      CHECK(rc == KW_OK && h.off[0] == 0 && h.off[1] == npol && h.off[2] == npol && h.off[3] == npol + 1, "hand-made offsets");
      CHECK(h.exc[5] == 0xA5A5A5A5u && h.exc[npol] == 0xA5A5A5A5u, "hand-made: the poisoned words survive as exceptions");
      uint32_t x = 0;
      CHECK(kw_packed_word(&h.p, 2, npol - 1, &x) == KW_OK && x == 0xA5A5A5A5u, "hand-made: word of the poisoned pair");
      // arguments
      Arrays m(3, npol, 8);
      m.p.rows = 4;
      CHECK(kw_debug_pack_words(env, all.data(), npol, KW_ORIGIN_VALIDATE, w.data(), 3, &m.p) == KW_E_ARG, "rows mismatch");
      const int32_t badp = np + 100000;
      Arrays q(1, 1, 1);
      CHECK(kw_debug_pack_words(env, &badp, 1, KW_ORIGIN_VALIDATE, w.data(), 1, &q.p) == KW_E_ARG, "policy out of range");
    }
    kw_env_destroy(env);
  }
  printf("cases %d failures %d\n", cases, failures);
  return failures ? 1 : 0;
}
