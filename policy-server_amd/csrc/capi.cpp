// capi.cpp — extern "C" implementation of include/kwgpu.h: argument checks, environment and batch
// lifetime, the host walk (kw_debug_host_walk) and the host epilogue (service.cpp). Uploads are
// upload.cpp's, passes and verdict read-back pass.cpp's, the bulk path bulk.cpp's; plan.cpp plans.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/kwgpu.h"
#include "automaton.hpp"
#include "batch.hpp"
#include "devbatch.hpp"
#include "env.hpp"
#include "groups.hpp"
#include "groupvm.hpp"
#include "kernels.hpp"
#include "knobs.hpp"
#include "metrics.hpp"
#include "pass.hpp"
#include "plan.hpp"
#include "service.hpp"
#include "slotplan.hpp"
#include "upload.hpp"
#include "yaml.hpp"

using namespace kw;

namespace {

void put_err(char* buf, size_t cap, const std::string& s) {
  if (!buf || cap == 0) return;
  size_t n = std::min(cap - 1, s.size());
  memcpy(buf, s.data(), n);
  buf[n] = 0;
}

int put_out(const std::string& s, char* buf, size_t cap, size_t* need) {
  if (need) *need = s.size() + 1;
  if (!buf || cap < s.size() + 1) return KW_E_NOSPACE;
  memcpy(buf, s.data(), s.size());
  buf[s.size()] = 0;
  return KW_OK;
}

}  // namespace

extern "C" {

const char* kw_version(void) { return "kwgpu 0.2 (gfx950)"; }

int kw_env_build(const char* json, size_t len, const kw_env_options* opts, kw_env** out, char* err, size_t errlen) {
  if (!json || !out) return KW_E_ARG;
  auto env = std::make_unique<kw_env>();
  Status st = build_env(json, len, opts ? opts->continue_on_errors != 0 : false,
                        opts ? opts->always_accept_namespace : nullptr, &env->e);
  if (!st.ok()) {
    put_err(err, errlen, st.message);
    return st.code;
  }
  int dev = opts ? opts->device : -1;
  if (int rc = upload_env(env.get(), dev)) {
    put_err(err, errlen, "cannot upload compiled tables to the device");
    return rc;
  }
  *out = env.release();
  return KW_OK;
}

int kw_env_build_yaml(const char* yaml, size_t len, const kw_env_options* opts, kw_env** out, char* err, size_t errlen) {
  if (!yaml || !out) return KW_E_ARG;
  std::string json, e;
  if (!yaml_to_json(yaml, len, &json, &e)) {  // read_policies_file: serde_yaml error -> boot failure
    put_err(err, errlen, "bootstrap failure: cannot parse policies: " + e);
    return KW_E_BOOTSTRAP;
  }
  return kw_env_build(json.data(), json.size(), opts, out, err, errlen);
}

int kw_yaml_to_json(const char* yaml, size_t len, char* buf, size_t cap, size_t* need) {
  if (!yaml && len) return KW_E_ARG;
  std::string json, e;
  if (!yaml_to_json(yaml, len, &json, &e)) {
    put_out(e, buf, cap, need);
    return KW_E_PAYLOAD;
  }
  return put_out(json, buf, cap, need);
}

int kw_env_serialize(const kw_env* env, void* buf, size_t cap, size_t* need) {
  if (!env) return KW_E_ARG;
  std::vector<uint8_t> s = env_serialize(env->e);
  if (need) *need = s.size();
  if (!buf || cap < s.size()) return KW_E_NOSPACE;
  memcpy(buf, s.data(), s.size());
  return KW_OK;
}

int kw_env_deserialize(const void* blob, size_t len, int device, kw_env** out, char* err, size_t errlen) {
  if (!blob || !out) return KW_E_ARG;
  auto env = std::make_unique<kw_env>();
  Status st = env_from_blob(blob, len, &env->e);
  if (!st.ok()) {
    put_err(err, errlen, st.message);
    return st.code;
  }
  if (int rc = upload_env(env.get(), device)) return rc;
  *out = env.release();
  return KW_OK;
}

void kw_env_destroy(kw_env* env) {
  if (!env) return;
  if (env->e.d_blob) {
    (void)hipSetDevice(env->e.device);
    (void)hipFree(env->e.d_blob);
  }
  delete env;
}

int kw_env_lookup(const kw_env* env, const char* id, size_t len, int32_t* idx) {
  if (!env || !id || !idx) return KW_E_ARG;
  return env_lookup(env->e, std::string(id, len), idx).code;
}

int kw_env_policy_count(const kw_env* env) { return env ? (int)env->e.nvisible : -1; }

int kw_env_policy_id(const kw_env* env, int32_t idx, char* buf, size_t cap) {
  if (!env || idx < 0 || (size_t)idx >= env->e.nvisible) return KW_E_ARG;
  return put_out(env->e.pol[(size_t)idx].id, buf, cap, nullptr);
}

int kw_env_is_group(const kw_env* env, int32_t idx) {
  if (!env || idx < 0 || (size_t)idx >= env->e.nvisible) return -1;
  return env->e.pol[(size_t)idx].is_group ? 1 : 0;
}

int kw_env_get_policy_mode(const kw_env* env, int32_t idx, int* mode) {
  if (!env || !mode || idx < 0 || (size_t)idx >= env->e.nvisible) return KW_E_ARG;
  const PolicyRec& r = env->e.pol[(size_t)idx];
  if (!r.registered) return KW_E_NOT_FOUND;
  *mode = r.mode;
  return KW_OK;
}

int kw_env_get_policy_allowed_to_mutate(const kw_env* env, int32_t idx, int* allowed) {
  if (!env || !allowed || idx < 0 || (size_t)idx >= env->e.nvisible) return KW_E_ARG;
  const PolicyRec& r = env->e.pol[(size_t)idx];
  if (!r.registered) return KW_E_NOT_FOUND;
  *allowed = r.allowed_to_mutate ? 1 : 0;
  return KW_OK;
}

int kw_env_should_always_accept_requests_made_inside_of_namespace(const kw_env* env, const char* ns, size_t len) {
  if (!env || !ns) return 0;
  return env->e.always_ns && *env->e.always_ns == std::string(ns, len) ? 1 : 0;
}

int kw_env_policy_initialization_error(const kw_env* env, int32_t idx, char* buf, size_t cap) {
  if (!env || idx < 0 || (size_t)idx >= env->e.nvisible) return -1;
  const PolicyRec& r = env->e.pol[(size_t)idx];
  if (!r.init_error) return 0;
  put_err(buf, cap, r.init_message);
  return 1;
}

int kw_env_validate_settings(const kw_env* env, int32_t idx, char* buf, size_t cap) {
  if (!env || idx < 0 || (size_t)idx >= env->e.nvisible) return KW_E_ARG;
  Status st = env_validate_settings(env->e, idx);
  if (!st.ok()) put_err(buf, cap, st.message);
  return st.code;
}

int kw_env_group_members(const kw_env* env, int32_t group, int32_t* out, int cap) {
  if (!env || group < 0 || (size_t)group >= env->e.nvisible) return -1;
  const PolicyRec& r = env->e.pol[(size_t)group];
  int n = (int)r.members.size();
  for (int i = 0; i < n && i < cap; ++i) out[i] = r.members[(size_t)i];
  return n;
}

int kw_pattern_match(int kind, const char* pat, const char* s, size_t len) {
  if (!pat || (!s && len)) return -1;
  std::vector<Pattern> ps{{(Pattern::Kind)kind, pat}};
  std::vector<Dfa> chain;  // one DFA, or the NFA element a pattern beyond the state budget becomes
  std::string err;
  if (!compile_column(ps, (size_t)1 << 30, kMaxDfaStates, &chain, &err) || chain.size() != 1) return -1;
  return chain[0].run((const uint8_t*)s, len) != 0 ? 1 : 0;
}

int kw_pattern_match_many(int kind, const char* pat, const char* const* subjects, const size_t* lens, size_t n,
                          int32_t* out) {
  if (!pat || (n && (!subjects || !lens || !out))) return -1;
  std::vector<Pattern> ps{{(Pattern::Kind)(kind & 0xff), pat}};
  std::vector<Dfa> chain;
  std::string err;
  if (kind & KW_PATTERN_FORCE_NFA) {
    chain.resize(1);
    if (!compile_nfa(ps[0], &chain[0], &err)) return -1;
  } else if (!compile_column(ps, (size_t)1 << 30, kMaxDfaStates, &chain, &err) || chain.size() != 1) {
    return -1;
  }
  for (size_t i = 0; i < n; ++i) out[i] = chain[0].run((const uint8_t*)subjects[i], lens[i]) != 0 ? 1 : 0;
  return KW_OK;
}

int kw_env_pattern_count(const kw_env* env, int col) {
  if (!env || col < 0 || col >= (int)NCOL) return -1;
  return (int)env->e.cols[col].pats.size();
}

int kw_env_pattern(const kw_env* env, int col, int idx, int* kind, char* buf, size_t cap) {
  if (!env || col < 0 || col >= (int)NCOL || idx < 0 || (size_t)idx >= env->e.cols[col].pats.size()) return KW_E_ARG;
  const Pattern& p = env->e.cols[col].pats[(size_t)idx];
  if (kind) *kind = (int)p.kind;
  return put_out(p.text, buf, cap, nullptr);
}

int kw_env_classify(const kw_env* env, int col, const char* key, size_t klen, const char* s, size_t len, uint32_t* pats,
                    int cap) {
  if (!env || col < 0 || col >= (int)NCOL || (!s && len) || (!key && klen)) return -1;
  const Env& E = env->e;
  std::vector<uint32_t> m;
  if (col == COL_LV) {
    const std::vector<uint32_t> kc = host_classes(E, COL_LK, (const uint8_t*)key, klen);
    const uint32_t k = kc.empty() ? 0u : kc[0];
    for (uint32_t c : host_value_classes(E, k, (const uint8_t*)s, len)) m.insert(m.end(), E.kv[c].matched.begin(), E.kv[c].matched.end());
  } else {
    for (uint32_t c : host_classes(E, (Col)col, (const uint8_t*)s, len))
      m.insert(m.end(), E.cols[col].class_pats[c].begin(), E.cols[col].class_pats[c].end());
  }
  std::sort(m.begin(), m.end());
  m.erase(std::unique(m.begin(), m.end()), m.end());
  for (int i = 0; i < (int)m.size() && i < cap; ++i) pats[i] = m[(size_t)i];
  return (int)m.size();
}

}  // extern "C"

namespace {
// Host restatement of the kernel's image-reference split (kernels.hip parse_image / image_part):
// the registry, effective tag (has_tag false for a digest-only reference) and normalised image.
void host_image_strings(const uint8_t* s, size_t n, std::string* reg, std::string* tag, bool* has_tag, std::string* norm) {
  const size_t NONE = (size_t)-1;
  size_t at = NONE, slash0 = NONE, slash1 = NONE, last_colon = NONE;
  bool dotcolon = false;
  for (size_t q = 0; q < n; ++q) {
    const uint8_t c = s[q];
    if (c == '@') {
      at = q;
      break;
    }
    if (c == '/') {
      if (slash0 == NONE) slash0 = q;
      else if (slash1 == NONE) slash1 = q;
    } else if (c == ':') {
      last_colon = q;
      if (slash0 == NONE) dotcolon = true;
    } else if (c == '.') {
      if (slash0 == NONE) dotcolon = true;
    }
  }
  auto eq = [&](size_t e, const char* lit) { return e == strlen(lit) && memcmp(s, lit, e) == 0; };
  const size_t name_end = at != NONE ? at : n;
  const bool is_reg = slash0 != NONE && (dotcolon || eq(slash0, "localhost"));
  const size_t rest_b = is_reg ? slash0 + 1 : 0;
  const size_t colon = (last_colon != NONE && last_colon >= rest_b) ? last_colon : NONE;
  const size_t path_end = colon != NONE ? colon : name_end;
  const size_t fsr = is_reg ? slash1 : slash0;
  const bool path_slash = fsr != NONE && fsr < path_end;
  const bool is_docker = !is_reg || eq(slash0, "docker.io");
  const bool eff_tag = colon != NONE || at == NONE;
  auto sub = [&](size_t b, size_t e) { return std::string((const char*)s + b, e - b); };
  *reg = is_reg ? sub(0, slash0) : std::string("docker.io");
  *has_tag = colon != NONE || at == NONE;
  *tag = colon != NONE ? sub(colon + 1, name_end) : (at == NONE ? std::string("latest") : std::string());
  *norm = *reg + "/";
  if (is_docker && !path_slash) *norm += "library/";
  *norm += sub(rest_b, path_end);
  if (eff_tag) *norm += ":" + (colon != NONE ? sub(colon + 1, name_end) : std::string("latest"));
  if (at != NONE) *norm += sub(at, n);
}

// Accessor of the sequential walks (slots.hpp) over host class arrays.
struct HostSrc {
  const Batch* b;
  ImgLayout il;
  uint32_t nlv_ = 0;
  std::vector<uint32_t> ns_, aa_, add_, drop_, lk_, lv_, img_;
  uint32_t rf(uint64_t r) const { return b->req_flags[r]; }
  uint32_t coff(uint64_t r) const { return b->ctr_off[r]; }
  uint32_t loff(uint64_t r) const { return b->lbl_off[r]; }
  uint32_t cflags(uint32_t c) const { return b->ctr_flags[c]; }
  uint32_t cadd(uint32_t c) const { return b->capadd_off[c]; }
  uint32_t cdrop(uint32_t c) const { return b->capdrop_off[c]; }
  uint32_t ns(uint64_t r) const { return ns_[r]; }
  uint32_t aa(uint32_t c) const { return aa_[c]; }
  uint32_t capadd(uint32_t k) const { return add_[k]; }
  uint32_t capdrop(uint32_t k) const { return drop_[k]; }
  uint32_t lk(uint32_t l) const { return lk_[l]; }
  uint32_t nlv() const { return nlv_; }
  uint32_t lv(uint32_t l, uint32_t j) const { return lv_[(size_t)l * nlv_ + j]; }
  uint32_t img(uint32_t c, uint32_t j) const { return img_[(size_t)c * il.n() + j]; }
};
}  // namespace

extern "C" {

int kw_debug_host_walk(const kw_env* env, const kw_batch* kb, const int32_t* policies, uint32_t npol, int origin,
                       uint32_t* out) {
  if (!env || !kb || (!policies && npol) || (!out && npol && kb->b.n)) return KW_E_ARG;
  const Env& E = env->e;
  const Batch& B = kb->b;
  const DevHeader* H = (const DevHeader*)E.blob.data();
  std::vector<SlotChunk> chunks;
  Status st = build_slot_chunks(E, policies, npol, origin, false, &chunks);
  if (!st.ok()) return st.code;
  // classification of every string with the blob's tables (env.cpp host_classes)
  HostSrc src;
  src.b = &B;
  src.il = {(H->col[COL_REG].lit_off ? 1u : 0u) + H->col[COL_REG].ndfa, (H->col[COL_TAG].lit_off ? 1u : 0u) + H->col[COL_TAG].ndfa,
            H->col[COL_IMG].ndfa};
  src.nlv_ = H->col[COL_LV].ndfa;
  auto one = [&](Col c, const StrCol& sc, size_t i) {
    const std::vector<uint32_t> v = host_classes(E, c, sc.bytes.data() + sc.off[i], sc.off[i + 1] - sc.off[i]);
    return v.empty() ? 0u : v[0];
  };
  for (size_t r = 0; r < B.n; ++r) src.ns_.push_back(one(COL_NS, B.ns, r));
  for (size_t c = 0; c < B.containers(); ++c) {
    src.aa_.push_back(one(COL_AA, B.ctr_aa, c));
    std::vector<uint32_t> ic;
    if (B.ctr_flags[c] & KW_CTR_HAS_IMAGE) {
      std::string reg, tag, norm;
      bool has_tag;
      host_image_strings(B.ctr_image.bytes.data() + B.ctr_image.off[c], B.ctr_image.off[c + 1] - B.ctr_image.off[c], &reg, &tag,
                         &has_tag, &norm);
      std::vector<uint32_t> r = host_classes(E, COL_REG, (const uint8_t*)reg.data(), reg.size());
      std::vector<uint32_t> t = has_tag ? host_classes(E, COL_TAG, (const uint8_t*)tag.data(), tag.size())
                                        : std::vector<uint32_t>(src.il.ntag, 0u);
      std::vector<uint32_t> m = host_classes(E, COL_IMG, (const uint8_t*)norm.data(), norm.size());
      ic.insert(ic.end(), r.begin(), r.end());
      ic.insert(ic.end(), t.begin(), t.end());
      ic.insert(ic.end(), m.begin(), m.end());
    }
    ic.resize(src.il.n(), 0u);
    src.img_.insert(src.img_.end(), ic.begin(), ic.end());
  }
  for (size_t k = 0; k < B.cap_add.n(); ++k) src.add_.push_back(one(COL_CAP, B.cap_add, k));
  for (size_t k = 0; k < B.cap_drop.n(); ++k) src.drop_.push_back(one(COL_CAP, B.cap_drop, k));
  for (size_t l = 0; l < B.labels(); ++l) {
    const uint32_t k = one(COL_LK, B.lbl_key, l);
    src.lk_.push_back(k);
    std::vector<uint32_t> v = host_value_classes(E, k, B.lbl_val.bytes.data() + B.lbl_val.off[l], B.lbl_val.off[l + 1] - B.lbl_val.off[l]);
    v.resize(src.nlv_, 0xffffu);
    src.lv_.insert(src.lv_.end(), v.begin(), v.end());
  }
  std::vector<uint32_t> vw(kSlots), va(kSlots);
  const ViolSink vs{vw.data(), va.data()};
  for (const SlotChunk& ch : chunks) {
    SlotView sv;
    sv.h = (const SlotHdr*)ch.rec.data();
    sv.base = ch.rec.data();
    const ColInfo* cols = (const ColInfo*)(ch.rec.data() + sv.h->o_cols);
    for (uint64_t r = 0; r < B.n; ++r) {
      const bool byp = is_bypass(B.req_flags[r], src.ns_[r], H->bypass_cls);
      uint64_t mut = 0;
      uint64_t rej = walk_privileged_caps(src, sv, r, vs, &mut);
      rej |= walk_apparmor_images(src, sv, r, vs);
      rej |= walk_labels(src, sv, r, vs);
      rej |= walk_namespace(src, sv, r, vs);
      for (uint32_t j = 0; j < ch.ncols; ++j) {
        uint64_t wide = 0;
        out[r * npol + ch.col0 + j] = byp ? kBypassWord : column_word(cols[j], rej, mut, sv.h->init, vw.data(), ch.rec.data(), &wide);
      }
    }
  }
  // wide groups: their members' words by the same host walk, then the jump code per row
  PassPlan wp;
  plan_wide_groups(E, std::vector<int32_t>(policies, policies + npol), nullptr, origin, &wp);
  const PassPlan::Wide& W = wp.wide;
  if (!W.groups.empty()) {
    const size_t nm = W.members.size();
    std::vector<uint32_t> mw(B.n * nm);
    if (int rc = kw_debug_host_walk(env, kb, W.members.data(), (uint32_t)nm, origin, mw.data())) return rc;
    std::vector<uint64_t> stack(std::max<uint32_t>(W.stack_words, 1));
    for (uint64_t r = 0; r < B.n; ++r)
      for (const WideGroupArgs& g : W.groups) {
        uint32_t* dst = out + r * npol + g.col;
        if (*dst == kBypassWord) continue;
        auto ok = [&](uint32_t m) {
          const uint32_t c = W.midx[g.midx_off + m];
          uint32_t x;
          if (c & kSplitMember) {
            const WideGroupArgs& a = W.aux[c & ~kSplitMember];
            x = combine_parts(a, (const uint32_t*)(W.progs.data() + a.prog_off),
                              [&](uint32_t t) { return mw[r * nm + W.midx[a.midx_off + t]]; });
          } else {
            x = mw[r * nm + c];
          }
          return (x & KW_V_ALLOWED) && !(x & KW_V_MUTATED);
        };
        uint64_t cz = 0;  // (the causes of a group of at most 15 members go into ARG)
        auto cause = [&](uint32_t m) {
          if (m < 64) cz |= 1ull << m;
        };
        auto rej = [&]() { return g.nmem <= 15 ? (g.rejb & 0xffffu) | ((uint32_t)cz << 16) : g.rejb; };
        if (g.kind == 1) {
          const int v = run_script_prog(W.progs.data() + g.prog_off, stack.data(), ok, cause);
          *dst = v == 1 ? g.okw : v == 0 ? rej() : g.errw;
          continue;
        }
        if (g.kind >= 2) {
          *dst = combine_parts(g, (const uint32_t*)(W.progs.data() + g.prog_off),
                               [&](uint32_t m) { return mw[r * nm + W.midx[g.midx_off + m]]; });
          continue;
        }
        const bool v = run_wide_prog(W.progs.data() + g.prog_off, g.prog_len, stack.data(), ok, cause);
        *dst = v ? g.okw : rej();
      }
  }
  return KW_OK;
}

int kw_batch_from_json(const char* const* docs, const size_t* lens, size_t n, int doc_kind, kw_batch** out,
                       int64_t* bad_row, char* err, size_t errlen) {
  if (!out || (n && (!docs || !lens))) return KW_E_ARG;
  auto kb = std::make_unique<kw_batch>();
  // contiguous document ranges flattened by up to KW_FLATTEN_THREADS threads (default: the
  // hardware threads, at most 16), then concatenated in order; the first bad row wins
  uint32_t nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (const int t = Knobs::num<KW_FLATTEN_THREADS>()) nt = (uint32_t)t;
  nt = (uint32_t)std::min<uint64_t>(nt, std::max<size_t>(1, n / 2048));
  std::vector<Batch> part(nt);
  std::vector<int64_t> bad(nt, -1);
  std::vector<std::string> perr(nt);
  auto work = [&](uint32_t t) {
    const size_t i0 = n * t / nt, i1 = n * (t + 1) / nt;
    for (size_t i = i0; i < i1; ++i)
      if (!flatten_document(docs[i], lens[i], doc_kind, &part[t], &perr[t])) {
        bad[t] = (int64_t)i;
        return;
      }
  };
  if (nt == 1) {
    work(0);
  } else {
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < nt; ++t) th.emplace_back(work, t);
    for (auto& x : th) x.join();
  }
  for (uint32_t t = 0; t < nt; ++t)
    if (bad[t] >= 0) {
      if (bad_row) *bad_row = bad[t];
      put_err(err, errlen, perr[t]);
      return KW_E_PAYLOAD;
    }
  if (nt == 1) {
    kb->b = std::move(part[0]);
  } else {
    for (uint32_t t = 0; t < nt; ++t) {
      kb->b.append(part[t]);
      part[t] = Batch();  // release as we go
    }
  }
  kb->b.finalize();
  *out = kb.release();
  return KW_OK;
}

int kw_batch_from_soa(const kw_soa* soa, kw_batch** out) {
  if (!soa || !out) return KW_E_ARG;
  auto kb = std::make_unique<kw_batch>();
  std::string e;
  if (!batch_from_soa(*soa, &kb->b, &e)) return KW_E_ARG;
  kb->b.finalize();
  *out = kb.release();
  return KW_OK;
}

int kw_batch_view(const kw_batch* b, kw_soa* view) {
  if (!b || !view) return KW_E_ARG;
  b->b.view(view);
  return KW_OK;
}

int kw_batch_to_device(kw_batch* kb, int device) { return upload_batch(kb, device, nullptr, true); }

int kw_batch_to_device_async(kw_batch* kb, int device, void* stream) {
  if (!stream) return KW_E_ARG;
  return upload_batch(kb, device, (hipStream_t)stream, false);
}

int kw_validate_host(const kw_env* env, kw_batch* b, const int32_t* policies, uint32_t npol, int origin, int device,
                     uint32_t* out, size_t count, uint32_t chunk_rows) {
  return validate_host(env, b, policies, npol, origin, device, out, count, chunk_rows);
}

int kw_host_alloc(int device, size_t bytes, void** out) {
  if (!out || device < 0) return KW_E_ARG;
  HIPCHK(hipSetDevice(device));
  *out = nullptr;
  HIPCHK(hipHostMalloc(out, std::max<size_t>(bytes, 1), hipHostMallocDefault));
  return KW_OK;
}

void kw_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int kw_stream_create(int device, void** stream) {
  if (!stream || device < 0) return KW_E_ARG;
  HIPCHK(hipSetDevice(device));
  hipStream_t s = nullptr;
  HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *stream = (void*)s;
  return KW_OK;
}

void kw_stream_destroy(void* stream) {
  if (stream) (void)hipStreamDestroy((hipStream_t)stream);
}

void kw_batch_destroy(kw_batch* b) { delete b; }

int kw_batch_pin_host(kw_batch* kb, int device) { return pin_host(kb, device); }

int kw_validate_batch(const kw_env* env, kw_batch* b, const int32_t* policies, uint32_t npol, int origin, void* stream) {
  PassPlan* plan = nullptr;
  if (int rc = validate_cached(env, b, policies, npol, origin, &plan)) return rc;
  return run_validate(env, b, *plan, origin, false, stream ? (hipStream_t)stream : b->dev->stream);
}

int kw_validate_rows(const kw_env* env, kw_batch* b, const int32_t* row_policy, int origin, void* stream) {
  if (!row_policy) return KW_E_ARG;
  PassPlan plan;
  if (int rc = validate_common(env, b, nullptr, 0, row_policy, origin, &plan)) return rc;
  return run_validate(env, b, plan, origin, false, stream ? (hipStream_t)stream : b->dev->stream);
}

int kw_batch_verdicts(kw_batch* b, uint32_t* host_out, size_t count) { return read_verdicts(b, host_out, count); }

int kw_debug_plan(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, uint32_t* out,
                  int cap) {
  if (!env || !kb || !out || cap < 8 || (!policies && npol)) return KW_E_ARG;
  // plan against a host view of the batch (no device memory, nothing launched), in the device-row
  // order kw_batch_to_device would give it
  std::unique_ptr<DeviceBatch> saved = std::move(kb->dev);
  kb->dev = host_view(kb);
  PassPlan plan;
  int rc = plan_pass(env, kb, policies, npol, nullptr, origin, Knobs::on<KW_BULK_DEBUG>(), &plan);
  const TileArgs& T = plan.geom;
  const uint32_t vals[8] = {T.lds_bytes, (uint32_t)plan.launches.size(), (uint32_t)plan.chunks.size(), T.lds_tables,
                            T.rows, T.cmax, T.kmax, T.lmax};
  for (int i = 0; i < 8; ++i) out[i] = rc == KW_OK ? vals[i] : 0u;
  if (cap >= 16) {  // regions: count, light rows, the first region's grid, the heavy region's LDS / rows / cmax / grid, scan regions
    const bool two = rc == KW_OK && plan.regions.size() == 2;
    const TileArgs* H = two ? &plan.regions[1].geom : nullptr;
    uint32_t more[8] = {rc == KW_OK ? (uint32_t)plan.regions.size() : 0u, (uint32_t)kb->dev->split,
                              rc == KW_OK ? plan.regions[0].grid : 0u, H ? H->lds_bytes : 0u, H ? H->rows : 0u,
                              H ? H->cmax : 0u, two ? plan.regions[1].grid : 0u, 0u};
    if (rc == KW_OK)  // regions launched as the wave-scan instantiation (kFeatRng), one bit each
      for (size_t k = 0; k < plan.regions.size() && k < 32; ++k) more[7] |= (plan.regions[k].geom.feat & kFeatRng) ? 1u << k : 0u;
    for (int i = 0; i < 8; ++i) out[8 + i] = more[i];
  }
  kb->dev->verdicts = nullptr;  // host memory: not the DeviceBatch's to free
  kb->dev = std::move(saved);
  return rc;
}

int kw_debug_copy_jobs(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, uint32_t* out,
                       size_t cap, size_t* needed) {
  if (!env || !kb || !needed || (!out && cap) || (!policies && npol)) return KW_E_ARG;
  std::unique_ptr<DeviceBatch> saved = std::move(kb->dev);
  kb->dev = host_view(kb);
  const DeviceBatch& D = *kb->dev;
  const Batch& B = dev_rows(kb);
  PassPlan plan;
  int rc = plan_pass(env, kb, policies, npol, nullptr, origin, false, &plan);
  std::vector<uint32_t> w;
  if (rc == KW_OK) {
    // a job's column by its base address: 0-5 the request / container arrays, then per staged
    // string column 6 + 2m its offsets and 7 + 2m its bytes
    const void* cols[kMaxCopyJobs] = {D.req_flags, D.ctr_off, D.lbl_off, D.ctr_flags, D.capadd_off, D.capdrop_off};
    for (int m = 0; m < (int)NSTR; ++m) cols[6 + 2 * m] = D.str[m].off, cols[7 + 2 * m] = D.str[m].bytes;
    w.push_back((uint32_t)plan.regions.size());
    for (const PassPlan::Region& rg : plan.regions) {
      const TileArgs& T = rg.geom;
      std::vector<TileDesc> desc;
      std::vector<uint32_t> ovf;
      const uint64_t ntiles = (rg.hi - rg.lo + T.rows - 1) / T.rows;
      if ((rc = build_descs(B, T, rg.lo, rg.hi, 0, ntiles, 4096, rg.grid, &desc, &ovf))) break;
      for (uint32_t v : {T.rows, T.njobs, (uint32_t)desc.size(), (uint32_t)ovf.size(), (uint32_t)rg.lo, (uint32_t)rg.hi, T.lds_bytes,
                         (uint32_t)D.split})
        w.push_back(v);
      for (uint32_t v : {T.o_rf, T.o_coff, T.o_loff, T.o_cflags, T.o_cadd, T.o_cdrop}) w.push_back(v);
      w.insert(w.end(), T.o_so, T.o_so + NSTR);
      w.insert(w.end(), T.o_sb, T.o_sb + NSTR);
      for (uint32_t j = 0; j < T.njobs; ++j) {
        const CopyJob& q = T.jobs[j];
        uint32_t col = 0xffffffffu;
        // (an unstaged column may share the host view's placeholder address: staged columns only)
        for (uint32_t c = 0; c < kMaxCopyJobs; ++c)
          if ((c < 6 || T.o_sb[(c - 6) / 2]) && q.base == (uint64_t)(uintptr_t)cols[c] && col == 0xffffffffu) col = c;
        for (uint32_t v : {col, copy_lds(q.code), (q.code & kCjX4) ? 16u : 4u, q.code}) w.push_back(v);
      }
      for (const TileDesc& d : desc) {
        const uint32_t* dw = (const uint32_t*)&d;
        w.insert(w.end(), dw, dw + sizeof(TileDesc) / 4);
        for (uint32_t j = 0; j < T.njobs; ++j) {
          const uint32_t code = T.jobs[j].code;
          const CopySpan sp = copy_span(code, dw[code & 31u], dw[(code >> 5) & 31u], d.r0hi);
          for (uint32_t v : {(uint32_t)sp.byte_off, (uint32_t)(sp.byte_off >> 32), sp.count}) w.push_back(v);
        }
      }
      w.insert(w.end(), ovf.begin(), ovf.end());
    }
  }
  kb->dev->verdicts = nullptr;  // host memory: not the DeviceBatch's to free
  kb->dev = std::move(saved);
  if (rc) return rc;
  *needed = w.size();
  if (cap < w.size()) return KW_E_NOSPACE;
  std::copy(w.begin(), w.end(), out);
  return KW_OK;
}

int kw_debug_tile_descs(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, uint32_t* out,
                        size_t cap, size_t* needed) {
  if (!env || !kb || !needed || (!out && cap) || (!policies && npol)) return KW_E_ARG;
  std::unique_ptr<DeviceBatch> saved = std::move(kb->dev);
  kb->dev = host_view(kb);
  const Batch& B = dev_rows(kb);
  PassPlan plan;
  int rc = plan_pass(env, kb, policies, npol, nullptr, origin, false, &plan);
  std::vector<uint32_t> w;
  if (rc == KW_OK) {
    std::vector<TileDesc> desc;
    std::vector<uint32_t> ovf;
    uint64_t at[2] = {0, 0}, nd[2] = {0, 0};
    rc = plan_descs(B, plan, &desc, &ovf, at, nd);  // what a resident pass uploads
    if (rc == KW_OK) {
      w.push_back((uint32_t)plan.regions.size());
      w.push_back(ovf[0]);
      for (size_t k = 0; k < plan.regions.size(); ++k) {
        const PassPlan::Region& rg = plan.regions[k];
        const TileArgs& T = rg.geom;
        const TileCostW W = tile_cost_weights(T.feat, T.need);
        for (uint32_t v : {T.rows, T.cmax, T.kmax, T.lmax, rg.grid, tile_slot(nd[k], rg.grid, 0).nx, rg.dyn ? 1u : 0u,
                           (uint32_t)nd[k], (uint32_t)rg.lo, (uint32_t)rg.hi})
          w.push_back(v);
        for (int m = 0; m < (int)NSTR; ++m) w.push_back(T.o_sb[m] ? 1u : 0u);
        w.insert(w.end(), T.sb_cap, T.sb_cap + NSTR);
        for (uint64_t i = at[k]; i < at[k] + nd[k]; ++i) {
          const uint32_t* dw = (const uint32_t*)&desc[i];
          w.insert(w.end(), dw, dw + sizeof(TileDesc) / 4);
          const uint64_t c = desc_cost(W, desc[i]);
          w.push_back((uint32_t)c);
          w.push_back((uint32_t)(c >> 32));
        }
      }
      w.insert(w.end(), ovf.begin() + 1, ovf.end());
    }
  }
  kb->dev->verdicts = nullptr;  // host memory: not the DeviceBatch's to free
  kb->dev = std::move(saved);
  if (rc) return rc;
  *needed = w.size();
  if (cap < w.size()) return KW_E_NOSPACE;
  std::copy(w.begin(), w.end(), out);
  return KW_OK;
}

uint64_t kw_debug_tile_cost(uint32_t feat, uint32_t need, uint32_t requests, uint32_t labels, uint32_t containers,
                            uint32_t capabilities) {
  return tile_cost(tile_cost_weights(feat, need), requests, labels, containers, capabilities);
}

int kw_debug_tile_slot(uint64_t ndesc, uint32_t grid, uint32_t workgroup, uint32_t tile, uint64_t* out) {
  if (!out || !grid || workgroup >= grid) return KW_E_ARG;
  const TileSlot s = tile_slot(ndesc, grid, workgroup);
  const uint64_t v[7] = {s.nx, s.xcd, s.slot, s.wpx, s.t_lo, s.t_hi, tile_at(s, tile)};
  std::copy(v, v + 7, out);
  return KW_OK;
}

int kw_debug_sched_tail(uint64_t ndesc, uint32_t grid, uint32_t workgroup, uint32_t rounds, uint64_t* out) {
  if (!out || !grid || workgroup >= grid) return KW_E_ARG;
  const TileSlot s = tile_slot(ndesc, grid, workgroup);
  const uint64_t tail = tile_tail_lo(s, rounds);
  const uint64_t first = s.t_lo + s.slot;
  const uint64_t v[7] = {s.t_lo, s.slot, s.wpx, tail > first ? (tail - first + s.wpx - 1) / s.wpx : 0, tail, s.t_hi,
                         tile_whole_rounds(ndesc, grid)};
  std::copy(v, v + 7, out);
  return KW_OK;
}

int kw_debug_sched_rounds(uint64_t ndesc, uint32_t grid, int dynamic, int* rounds) {
  if (!rounds || !grid) return KW_E_ARG;
  *rounds = sched_static_rounds(ndesc, grid, dynamic != 0);
  return KW_OK;
}

int kw_debug_last_launches(const kw_batch* kb, int64_t* out, size_t cap, size_t* needed) {
  if (!kb || !kb->dev || !needed || (!out && cap)) return KW_E_ARG;
  const std::vector<int64_t>& v = kb->dev->last_launches;
  *needed = v.size();
  if (cap < v.size()) return KW_E_NOSPACE;
  std::copy(v.begin(), v.end(), out);
  return KW_OK;
}

int kw_debug_last_kernels(const kw_batch* kb, uint32_t* out, size_t cap, size_t* needed) {
  if (!kb || !kb->dev || !needed || (!out && cap)) return KW_E_ARG;
  const std::vector<uint32_t>& v = kb->dev->last_kernels;
  *needed = v.size();
  if (cap < v.size()) return KW_E_NOSPACE;
  std::copy(v.begin(), v.end(), out);
  return KW_OK;
}

int kw_debug_prod_shape(uint32_t feat, int lds_tables, uint32_t debug, uint32_t nchunk, int rows_mode, int prefetch,
                        uint32_t ncols, int vec4, int timing) {
  TileArgs t;
  memset(&t, 0, sizeof(t));
  t.feat = feat;
  t.ctr_ranges = (feat & kFeatRng) ? 1u : 0u;
  t.lds_tables = lds_tables ? 1u : 0u;
  t.debug = debug;
  t.nchunk = nchunk;
  t.rows_mode = rows_mode ? 1u : 0u;
  t.prefetch = prefetch ? 1u : 0u;
  t.chunk[0].ncols = ncols;
  t.chunk[0].vec4 = vec4 ? 1u : 0u;
  return tile_prod_shape(t, timing != 0) ? 1 : 0;
}

int kw_debug_plan_kernels(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, uint32_t* out,
                          size_t cap, size_t* needed) {
  if (!env || !kb || !needed || (!out && cap) || (!policies && npol)) return KW_E_ARG;
  std::unique_ptr<DeviceBatch> saved = std::move(kb->dev);
  kb->dev = host_view(kb);
  PassPlan plan;
  const int rc = plan_pass(env, kb, policies, npol, nullptr, origin, false, &plan);
  std::vector<uint32_t> w;
  if (rc == KW_OK)
    for (const TileArgs& t : plan.tiles) w.push_back(tile_kernel_kind(t, (t.debug & 512u) != 0));
  kb->dev->verdicts = nullptr;  // host memory: not the DeviceBatch's to free
  kb->dev = std::move(saved);
  if (rc) return rc;
  *needed = w.size();
  if (cap < w.size()) return KW_E_NOSPACE;
  std::copy(w.begin(), w.end(), out);
  return KW_OK;
}

int kw_debug_last_variants(const kw_batch* kb, uint32_t* out, size_t cap, size_t* needed) {
  if (!kb || !kb->dev || !needed || (!out && cap)) return KW_E_ARG;
  const std::vector<uint32_t>& v = kb->dev->last_variants;
  *needed = v.size();
  if (cap < v.size()) return KW_E_NOSPACE;
  std::copy(v.begin(), v.end(), out);
  return KW_OK;
}

int kw_debug_plan_variants(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, uint32_t* out,
                           size_t cap, size_t* needed) {
  if (!env || !kb || !needed || (!out && cap) || (!policies && npol)) return KW_E_ARG;
  std::unique_ptr<DeviceBatch> saved = std::move(kb->dev);
  kb->dev = host_view(kb);
  PassPlan plan;
  const int rc = plan_pass(env, kb, policies, npol, nullptr, origin, false, &plan);
  std::vector<uint32_t> w;
  if (rc == KW_OK)
    for (const TileArgs& t : plan.tiles) w.push_back(tile_variant_word(tile_variant(t, (t.debug & 512u) != 0)));
  kb->dev->verdicts = nullptr;  // host memory: not the DeviceBatch's to free
  kb->dev = std::move(saved);
  if (rc) return rc;
  *needed = w.size();
  if (cap < w.size()) return KW_E_NOSPACE;
  std::copy(w.begin(), w.end(), out);
  return KW_OK;
}

uint32_t kw_debug_resolve_variant(uint32_t variant) { return tile_variant_word(tile_resolve(tile_variant_of(variant))); }

int kw_debug_reorder(const kw_batch* kb, uint64_t* perm, size_t cap, uint64_t* split, kw_batch** out) {
  if (!kb || !split || !out || (!perm && kb->b.n) || cap < kb->b.n) return KW_E_ARG;
  std::vector<uint64_t> p;
  *split = split_rows(kb->b, &p);
  if (!*split) {
    p.resize(kb->b.n);
    for (uint64_t r = 0; r < kb->b.n; ++r) p[r] = r;
  }
  auto nb = std::make_unique<kw_batch>();
  RowOrder o;
  permute_batch(kb->b, p, &nb->b, /*with_bytes=*/true, &o);
  std::copy(p.begin(), p.end(), perm);
  *out = nb.release();
  return KW_OK;
}

int kw_batch_group_causes(const kw_batch* b, uint64_t row, int32_t policy, uint32_t verdict, uint64_t* words,
                          size_t nwords, size_t* needed) {
  if (!b || (!words && nwords)) return KW_E_ARG;
  if (KW_REASON(verdict) != KW_R_GROUP) return KW_E_ARG;
  const WideData& W = b->b.wide;
  uint32_t bw = 0;
  const uint64_t* big = W.lookup_big(row, policy, &bw);
  uint64_t one = KW_ARG(verdict);
  if (!big && KW_ARG(verdict) == kArgWide && !W.lookup(row, policy, &one)) return KW_E_NOT_FOUND;
  const size_t n = big ? bw : 1u;
  if (needed) *needed = n;
  if (nwords < n) return KW_E_NOSPACE;
  for (size_t k = 0; k < n; ++k) words[k] = big ? big[k] : one;
  return KW_OK;
}

int kw_batch_wide_arg(const kw_batch* b, uint64_t row, int32_t policy, uint64_t* value) {
  if (!b || !value) return KW_E_ARG;
  return b->b.wide.lookup(row, policy, value) ? KW_OK : KW_E_NOT_FOUND;
}

int kw_batch_messages(kw_batch* b, const kw_env* env, const int32_t* policies, uint32_t npol, const uint64_t* rows,
                      const uint32_t* cols, size_t n, kw_messages* out) {
  if (!b || !env || !out || (npol && !policies)) return KW_E_ARG;
  return batch_messages(b, env, policies, npol, rows, cols, n, out);
}

int kw_debug_messages_words(const kw_env* env, const kw_batch* b, const int32_t* policies, uint32_t npol, const uint32_t* words,
                            uint64_t nrows, const uint64_t* rows, const uint32_t* cols, size_t n, int how, kw_messages* out) {
  if (!b || !env || !out || (npol && !policies)) return KW_E_ARG;
  return debug_messages_words(env, b, policies, npol, words, nrows, rows, cols, n, how, out);
}

int kw_debug_messages_stats(const kw_batch* b, uint64_t* out) { return debug_messages_stats(b, out); }

int kw_batch_responses(kw_batch* b, const kw_env* env, const int32_t* policies, uint32_t npol, const uint64_t* rows,
                       const uint32_t* cols, size_t n, kw_responses* out) {
  if (!b || !env || !out || (npol && !policies)) return KW_E_ARG;
  return batch_responses(b, env, policies, npol, rows, cols, n, out);
}

int kw_debug_responses_words(const kw_env* env, const kw_batch* b, const int32_t* policies, uint32_t npol, const uint32_t* words,
                             uint64_t nrows, const uint64_t* rows, const uint32_t* cols, size_t n, int how, kw_responses* out) {
  if (!b || !env || !out || (npol && !policies)) return KW_E_ARG;
  return debug_responses_words(env, b, policies, npol, words, nrows, rows, cols, n, how, out);
}

int kw_debug_responses_stats(const kw_batch* b, uint64_t* out) { return debug_responses_stats(b, out); }

int kw_batch_set_patch_shape(kw_batch* b, const uint32_t* ctr_place, uint64_t n_containers, const uint8_t* req_place,
                             uint64_t n_requests) {
  return batch_set_patch_shape(b, ctr_place, n_containers, req_place, n_requests);
}

int kw_batch_patch_shape(const kw_batch* b, uint32_t* ctr_place, uint64_t n_containers, uint8_t* req_place, uint64_t n_requests) {
  return batch_patch_shape(b, ctr_place, n_containers, req_place, n_requests);
}

int kw_format_patch(const kw_env* env, const kw_batch* b, uint64_t row, int32_t policy, uint32_t verdict, int form, char* buf,
                    size_t cap, size_t* need) {
  if (!env || !b || row >= b->b.n || policy < 0 || (size_t)policy >= env->e.nvisible || (form != KW_PATCH_OPS && form != KW_PATCH_RESPONSE))
    return KW_E_ARG;
  std::string out;
  Status st = format_patch(env->e, b->b, row, policy, verdict, form, &out);
  if (!st.ok()) {
    put_out(st.message, buf, cap, need);
    return st.code;
  }
  return put_out(out, buf, cap, need);
}

int kw_batch_patches(kw_batch* b, const kw_env* env, const int32_t* policies, uint32_t npol, const uint64_t* rows,
                     const uint32_t* cols, size_t n, int form, kw_responses* out) {
  if (!b || !env || !out || (npol && !policies)) return KW_E_ARG;
  return batch_patches(b, env, policies, npol, rows, cols, n, form, out);
}

int kw_debug_patches_words(const kw_env* env, const kw_batch* b, const int32_t* policies, uint32_t npol, const uint32_t* words,
                           uint64_t nrows, const uint64_t* rows, const uint32_t* cols, size_t n, int form, int how,
                           kw_responses* out) {
  if (!b || !env || !out || (npol && !policies)) return KW_E_ARG;
  return debug_patches_words(env, b, policies, npol, words, nrows, rows, cols, n, form, how, out);
}

int kw_debug_patches_stats(const kw_batch* b, uint64_t* out) { return debug_patches_stats(b, out); }

int kw_validate_timed(const kw_env* env, kw_batch* b, const int32_t* policies, uint32_t npol, int origin, int warmup,
                      int reps, kw_timing* out) {
  return validate_timed(env, b, policies, npol, origin, warmup, reps, out);
}

int kw_format_response(const kw_env* env, const kw_batch* b, uint64_t row, int32_t policy, uint32_t verdict,
                       const uint32_t* member_verdicts, char* buf, size_t cap, size_t* need) {
  if (!env || !b || row >= b->b.n || policy < 0 || (size_t)policy >= env->e.nvisible) return KW_E_ARG;
  std::string out;
  Status st = format_response(env->e, b->b, row, policy, verdict, member_verdicts, &out);
  if (!st.ok()) {
    put_out(st.message, buf, cap, need);
    return st.code;
  }
  return put_out(out, buf, cap, need);
}

int kw_format_response_doc(const kw_env* env, const kw_batch* b, uint64_t row, int32_t policy, uint32_t verdict,
                           const uint32_t* member_verdicts, const char* doc, size_t doc_len, int doc_kind, char* buf,
                           size_t cap, size_t* need) {
  if (!env || !b || row >= b->b.n || policy < 0 || (size_t)policy >= env->e.nvisible || (!doc && doc_len))
    return KW_E_ARG;
  std::string out;
  Status st = format_response(env->e, b->b, row, policy, verdict, member_verdicts, &out, doc, doc_len, doc_kind);
  if (!st.ok()) {
    put_out(st.message, buf, cap, need);
    return st.code;
  }
  return put_out(out, buf, cap, need);
}

int kw_evaluate(const kw_env* env, const char* policy_id, const char* doc, size_t doc_len, int doc_kind, int origin,
                char* buf, size_t cap, size_t* need) {
  if (!env || !policy_id || !doc) return KW_E_ARG;
  const Env& E = env->e;
  int32_t idx;
  Status st = env_lookup(E, policy_id, &idx);  // service.rs:37 + PolicyNotFound
  if (!st.ok()) {
    put_out(st.message, buf, cap, need);
    return st.code;
  }
  kw_batch* kb = nullptr;
  char err[512];
  int rc = kw_batch_from_json(&doc, &doc_len, 1, doc_kind, &kb, nullptr, err, sizeof(err));
  if (rc) {
    put_out(err, buf, cap, need);
    return rc;
  }
  std::unique_ptr<kw_batch> hold(kb);
  if (E.device < 0) {
    put_out("engine has no device: the hot path runs only on the GPU", buf, cap, need);
    return KW_E_DEVICE;
  }
  if ((rc = kw_batch_to_device(kb, E.device))) return rc;
  std::vector<int32_t> pols{idx};
  const PolicyRec& P = E.pol[(size_t)idx];
  for (int32_t m : P.members) pols.push_back(m);
  if ((rc = kw_validate_batch(env, kb, pols.data(), (uint32_t)pols.size(), origin, nullptr))) return rc;
  std::vector<uint32_t> v(pols.size());
  if ((rc = kw_batch_verdicts(kb, v.data(), v.size()))) return rc;
  std::string out;
  st = format_response(E, kb->b, 0, idx, v[0], v.size() > 1 ? v.data() + 1 : nullptr, &out, doc, doc_len, doc_kind);
  if (!st.ok()) {
    put_out(st.message, buf, cap, need);
    return st.code;
  }
  return put_out(out, buf, cap, need);
}

int kw_service_constraints(uint32_t in, int mode, int allowed_to_mutate, uint32_t* out_flags) {
  // validation_response_with_constraints (service.rs:160-208); bit0 allowed, bit1 patch, bit2 status
  uint32_t o = in;
  int fst;
  if (mode == KW_MODE_MONITOR) {
    o = 1u;
    fst = KW_FST_NONE;
  } else if ((in & 2u) && !allowed_to_mutate) {
    o = 4u;
    fst = KW_FST_MUTATION_REFUSED;
  } else {
    fst = (in & 4u) ? KW_FST_VANILLA : KW_FST_NONE;
  }
  if (out_flags) *out_flags = o;
  return fst;
}

}  // extern "C"

// ---- metrics (metrics.hpp)
struct kw_metrics {
  kw::Metrics m;
};

kw_metrics* kw_metrics_create(void) { return new (std::nothrow) kw_metrics(); }
void kw_metrics_destroy(kw_metrics* m) { delete m; }

int kw_metrics_record(kw_metrics* m, const kw_env* env, const kw_batch* b, const uint64_t* rows,
                      const int32_t* policies, const uint32_t* verdicts, const uint64_t* latency_ms, size_t n,
                      int origin) {
  if (!m || !env || !b || (n && (!rows || !policies || !verdicts || !latency_ms))) return KW_E_ARG;
  if (origin != KW_ORIGIN_VALIDATE && origin != KW_ORIGIN_AUDIT) return KW_E_ARG;
  for (size_t i = 0; i < n; ++i)
    if (rows[i] >= b->b.n || policies[i] < 0 || (size_t)policies[i] >= env->e.nvisible) return KW_E_ARG;
  for (size_t i = 0; i < n; ++i) m->m.record(env->e, b->b, rows[i], policies[i], verdicts[i], origin, latency_ms[i]);
  return KW_OK;
}

int kw_metrics_add_outcomes(kw_metrics* m, const kw_env* env, const kw_batch* b, const int32_t* policies, uint32_t npol,
                            int origin, uint64_t latency_ms, const uint64_t* first_row, uint32_t ngroups,
                            const uint64_t* counts) {
  if (!m || !env || !b || !policies || npol == 0 || (ngroups && (!first_row || !counts))) return KW_E_ARG;
  if (origin != KW_ORIGIN_VALIDATE && origin != KW_ORIGIN_AUDIT) return KW_E_ARG;
  return m->m.add_outcomes(env->e, b->b, policies, npol, origin, latency_ms, first_row, ngroups, counts) ? KW_OK : KW_E_ARG;
}

int kw_metrics_record_pass(kw_metrics* m, const kw_env* env, kw_batch* b, const int32_t* policies, uint32_t npol,
                           int origin, uint64_t latency_ms) {
  uint64_t rows = 0;
  uint32_t rw = 0;
  if (!m || !env || !policies || kw_batch_last_pass(b, &rows, &rw) != KW_OK) return KW_E_ARG;
  if (origin != KW_ORIGIN_VALIDATE && origin != KW_ORIGIN_AUDIT) return KW_E_ARG;
  // an all-pairs pass over these policies: a kw_validate_rows pass has a policy per row in its one column
  if (b->dev->last_rows_mode || rw != npol || rows != b->b.n) return KW_E_ARG;
  uint32_t ngroups = 0;
  std::vector<uint32_t> row_group((size_t)rows);
  (void)kw_batch_attribute_groups(b, nullptr, nullptr, 0, &ngroups);  // (the count; built once per batch)
  std::vector<uint64_t> first_row(ngroups);
  if (int rc = kw_batch_attribute_groups(b, row_group.data(), first_row.data(), first_row.size(), &ngroups)) return rc;
  if (ngroups == 0) return KW_OK;  // no rows
  std::vector<uint64_t> counts((size_t)ngroups * KW_OUT_N * npol);
  if (int rc = kw_batch_outcomes(b, row_group.data(), ngroups, counts.data())) return rc;
  return kw_metrics_add_outcomes(m, env, b, policies, npol, origin, latency_ms, first_row.data(), ngroups, counts.data());
}

int kw_metrics_render(const kw_metrics* m, char* buf, size_t cap, size_t* need) {
  if (!m) return KW_E_ARG;
  return put_out(m->m.render(), buf, cap, need);
}

void kw_metrics_reset(kw_metrics* m) {
  if (m) m->m.reset();
}
