// patches.cpp — the JSONPatch of accepted mutations from columns (include/kwgpu.h): the patches'
// table from (env, policies); kw_format_patch, one pair's ops or response from the host columns,
// written plainly with std::string as capabilities_patch (service.cpp) is (the reference of the
// diagnostics, and the call of a host caller that holds columns and no documents);
// kw_batch_patches, which uploads the shape columns and the uids on first use and runs the items
// through the rounds of the responses (rounds.hpp); the two host renderers of the diagnostic. The
// arithmetic is patches.hpp's, the kernels reports.hip's.
#include "patches.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "json.hpp"
#include "knobs.hpp"
#include "lastpass.hpp"
#include "reports.hpp"
#include "rounds.hpp"
#include "service.hpp"
#include "upload.hpp"

namespace kw {
namespace {

static_assert(sizeof(PatchCol) == 20 && sizeof(PatchName) == 16 && sizeof(PatchHead) == 16, "patches records");

// The patches' table of a pass over `policies` (patch_build_table); KW_E_ARG for an index outside
// the visible policies. A split policy's visible record holds its whole lists.
int patches_table(const Env& E, const int32_t* policies, uint32_t npol, std::vector<uint64_t>* block) {
  if (npol && !policies) return KW_E_ARG;
  std::vector<PatchColSource> cols(npol);
  for (uint32_t c = 0; c < npol; ++c) {
    if (policies[c] < 0 || (size_t)policies[c] >= E.nvisible) return KW_E_ARG;
    const PolicyRec& P = E.pol[(size_t)policies[c]];
    cols[c].capabilities = P.family == FAM_CAPABILITIES;
    cols[c].required_drop = P.lists[1];
    cols[c].default_add = P.lists[2];
  }
  *block = patch_build_table(cols);
  return KW_OK;
}

PatchCols host_patch_cols(const Batch& B) {
  PatchCols C{};
  C.rows = B.n;
  C.nctr = B.containers();
  C.ctr_off = B.ctr_off.data();
  C.capadd_off = B.capadd_off.data();
  C.capdrop_off = B.capdrop_off.data();
  C.ctr_flags = B.ctr_flags.data();
  C.add = DigestStr{B.cap_add.off.data(), B.cap_add.bytes.data(), B.cap_add.n()};
  C.drop = DigestStr{B.cap_drop.off.data(), B.cap_drop.bytes.data(), B.cap_drop.n()};
  C.uid = DigestStr{B.uid.off.data(), B.uid.bytes.data(), B.uid.n()};
  C.ctr_place = B.ctr_place.size() == B.containers() ? B.ctr_place.data() : nullptr;
  C.req_place = B.req_place.size() == B.n ? B.req_place.data() : nullptr;
  return C;
}

std::string base64(const std::string& in) {
  static const char* T = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  std::string o;
  for (size_t i = 0; i < in.size(); i += 3) {
    const size_t m = std::min<size_t>(3, in.size() - i);
    uint32_t x = 0;
    for (size_t k = 0; k < 3; ++k) x = (x << 8) | (k < m ? (uint8_t)in[i + k] : 0u);
    o += T[x >> 18];
    o += T[(x >> 12) & 63];
    o += m > 1 ? T[(x >> 6) & 63] : '=';
    o += m > 2 ? T[x & 63] : '=';
  }
  return o;
}

std::string json_list(const std::vector<std::string>& l) {
  std::string o = "[";
  for (size_t i = 0; i < l.size(); ++i) {
    if (i) o += ",";
    json_escape(&o, l[i]);
  }
  return o + "]";
}

// The shape columns to the device in device order (a split batch: the rows through the upload's
// permutation, the containers in the order of those rows).
int upload_places(kw_batch* kb, hipStream_t s) {
  DeviceBatch& D = *kb->dev;
  const Batch& B = kb->b;
  const uint64_t nc = B.containers();
  if (B.ctr_place.size() != nc || B.req_place.size() != B.n) return KW_E_ARG;
  const size_t b_ctr = round_up((size_t)(nc + 1) * 4, 256), total = b_ctr + round_up((size_t)B.n + 16, 256);
  BlockLease h;
  HIPCHK(h.alloc(host_pool(), D.device, total));
  uint32_t* cp = (uint32_t*)h.p;
  uint8_t* rp = (uint8_t*)h.p + b_ctr;
  memset(h.p, 0, total);
  if (D.split && D.perm.size() == B.n) {
    uint64_t e = 0;
    for (uint64_t d = 0; d < B.n; ++d) {
      const uint64_t r = D.perm[d];
      rp[d] = B.req_place[r];
      for (uint32_t c = B.ctr_off[r]; c < B.ctr_off[r + 1]; ++c) cp[e++] = B.ctr_place[c];
    }
    if (e != nc) return KW_E_ENGINE;
  } else {
    if (nc) memcpy(cp, B.ctr_place.data(), (size_t)nc * 4);
    if (B.n) memcpy(rp, B.req_place.data(), (size_t)B.n);
  }
  void* d = nullptr;
  HIPCHK(dev_pool().alloc(D.device, total, &d));
  const hipError_t e1 = hipMemcpyAsync(d, h.p, total, hipMemcpyHostToDevice, s);
  const hipError_t e2 = hipStreamSynchronize(s);  // (the staging block returns to its pool below)
  if (e1 != hipSuccess || e2 != hipSuccess) {
    dev_pool().release(D.device, d, total);
    return KW_E_DEVICE;
  }
  D.places = (uint8_t*)d;
  D.places_bytes = total;
  D.ctr_place = (const uint32_t*)D.places;
  D.req_place = D.places + b_ctr;
  return KW_OK;
}

bool form_ok(int form) { return form == KW_PATCH_OPS || form == KW_PATCH_RESPONSE; }

}  // namespace

// One pair's patch from the host columns: capabilities_patch's steps over the container's ranges.
Status format_patch(const Env& env, const Batch& b, uint64_t row, int32_t pidx, uint32_t v, int form, std::string* out) {
  const PolicyRec& P = env.pol[(size_t)pidx];
  out->clear();
  if (!(v & KW_F_PATCH)) return {KW_E_ARG, "the verdict carries no patch (KW_F_PATCH)"};
  if (P.family != FAM_CAPABILITIES) return {KW_E_ARG, "mutation by a non-mutating policy family: no patch is defined for " + P.id};
  if (b.req_place.size() != b.n || b.ctr_place.size() != b.containers() || b.req_place[row] == KW_PP_UNKNOWN)
    return {KW_E_ARG, "the Pod-spec pointer of request " + std::to_string(row) + " is unknown (kw_batch_set_patch_shape)"};
  static const char* kPointer[] = {"", "", "/spec", "/spec/template/spec", "/spec/jobTemplate/spec/template/spec"};
  const uint32_t pp = b.req_place[row];
  const uint32_t cb = b.ctr_off[row], ce = b.ctr_off[row + 1];
  for (uint32_t c = cb; c < ce; ++c)
    if (KW_PS_SHAPE(b.ctr_place[c]) == KW_PS_UNKNOWN || KW_PS_SHAPE(b.ctr_place[c]) > KW_PS_MAX)
      return {KW_E_ARG, "the patch shape of container " + std::to_string(c - cb) + " of request " + std::to_string(row) +
                            " is unknown (kw_batch_set_patch_shape)"};
  auto uniq = [](const std::vector<std::string>& l) {
    std::vector<std::string> o;
    for (const auto& x : l)
      if (std::find(o.begin(), o.end(), x) == o.end()) o.push_back(x);
    return o;
  };
  const std::vector<std::string> reqd = uniq(P.lists[1]), defa = uniq(P.lists[2]);
  std::string ops = "[";
  auto op = [&](const std::string& path, const std::string& value) {
    if (ops.size() > 1) ops += ",";
    ops += "{\"op\":\"add\",\"path\":";
    json_escape(&ops, path);
    ops += ",\"value\":" + value + "}";
  };
  for (uint32_t c = cb; c < ce && pp != KW_PP_NONE; ++c) {
    auto has = [&](const StrCol& col, const std::vector<uint32_t>& off, const std::string& x) {
      for (uint32_t k = off[c]; k < off[c + 1]; ++k)
        if (col.at(k) == x) return true;
      return false;
    };
    std::vector<std::string> mdrop, madd;
    if (!has(b.cap_drop, b.capdrop_off, "ALL"))
      for (const auto& x : reqd)
        if (!has(b.cap_drop, b.capdrop_off, x)) mdrop.push_back(x);
    for (const auto& x : defa)
      if (!has(b.cap_add, b.capadd_off, x) && !has(b.cap_drop, b.capdrop_off, x)) madd.push_back(x);
    if (mdrop.empty() && madd.empty()) continue;
    const uint32_t shape = KW_PS_SHAPE(b.ctr_place[c]);
    const char* ln = (b.ctr_flags[c] & KW_CTR_INIT) ? "initContainers" : (b.ctr_flags[c] & KW_CTR_EPHEMERAL) ? "ephemeralContainers" : "containers";
    const std::string base = std::string(kPointer[pp]) + "/" + ln + "/" + std::to_string(KW_PS_INDEX(b.ctr_place[c])) + "/securityContext";
    std::string cap_obj = "{";
    if (!madd.empty()) cap_obj += "\"add\":" + json_list(madd);
    if (!mdrop.empty()) cap_obj += std::string(madd.empty() ? "" : ",") + "\"drop\":" + json_list(mdrop);
    cap_obj += "}";
    if (shape == KW_PS_NO_SC) {
      op(base, "{\"capabilities\":" + cap_obj + "}");
    } else if (shape == KW_PS_NO_CAPS) {
      op(base + "/capabilities", cap_obj);
    } else {
      for (int is_add = 1; is_add >= 0; --is_add) {
        const std::vector<std::string>& l = is_add ? madd : mdrop;
        if (l.empty()) continue;
        const std::string lp = base + "/capabilities/" + (is_add ? "add" : "drop");
        const bool is_arr = ((shape - KW_PS_CAPS) & (is_add ? KW_PS_ADD_ARRAY : KW_PS_DROP_ARRAY)) != 0;
        if (!is_arr) {
          op(lp, json_list(l));
        } else {
          for (const auto& x : l) {
            std::string q;
            json_escape(&q, x);
            op(lp + "/-", q);
          }
        }
      }
    }
  }
  ops += "]";
  if (form == KW_PATCH_OPS) {
    *out = std::move(ops);
    return {};
  }
  out->append("{\"uid\":");
  json_escape(out, b.uid.at(row));
  out->append(",\"allowed\":true,\"patchType\":\"JSONPatch\",\"patch\":");
  json_escape(out, base64(ops));
  out->append("}");
  return {};
}

int batch_set_patch_shape(kw_batch* kb, const uint32_t* ctr_place, uint64_t nc, const uint8_t* req_place, uint64_t nr) {
  if (!kb || nc != kb->b.containers() || nr != kb->b.n || (nc && !ctr_place) || (nr && !req_place)) return KW_E_ARG;
  for (uint64_t c = 0; c < nc; ++c)
    if (KW_PS_SHAPE(ctr_place[c]) > KW_PS_MAX) return KW_E_ARG;
  for (uint64_t r = 0; r < nr; ++r)
    if (req_place[r] > KW_PP_CRONJOB) return KW_E_ARG;
  kb->b.ctr_place.assign(ctr_place, ctr_place + nc);
  kb->b.req_place.assign(req_place, req_place + nr);
  if (kb->dev && kb->dev->places) {  // the device copy is of the old shape: no kernel reads it after the drain
    DeviceBatch& D = *kb->dev;
    HIPCHK(hipSetDevice(D.device));
    if (D.stream) HIPCHK(hipStreamSynchronize(D.stream));
    if (D.cur && D.cur != D.stream) HIPCHK(hipStreamSynchronize(D.cur));
    dev_pool().release(D.device, D.places, D.places_bytes);
    D.places = nullptr;
    D.places_bytes = 0;
    D.ctr_place = nullptr;
    D.req_place = nullptr;
  }
  return KW_OK;
}

int batch_patch_shape(const kw_batch* kb, uint32_t* ctr_place, uint64_t nc, uint8_t* req_place, uint64_t nr) {
  if (!kb || nc != kb->b.containers() || nr != kb->b.n || kb->b.ctr_place.size() != nc || kb->b.req_place.size() != nr) return KW_E_ARG;
  if (ctr_place && nc) memcpy(ctr_place, kb->b.ctr_place.data(), (size_t)nc * 4);
  if (req_place && nr) memcpy(req_place, kb->b.req_place.data(), (size_t)nr);
  return KW_OK;
}

int batch_patches(kw_batch* b, const kw_env* env, const int32_t* policies, uint32_t npol, const uint64_t* rows, const uint32_t* cols,
                  size_t n, int form, kw_responses* out) {
  if (!out) return KW_E_ARG;
  out->bytes = out->nhost = 0;
  LastPass F(b, LastPass::kWholeBatch);
  if (!env || !F.ok() || npol != F.npol || !form_ok(form)) return KW_E_ARG;
  const uint64_t nrows = F.rows;
  DeviceBatch& D = *F.dev;
  if (!responses_out_ok(out, rows, cols, n)) return KW_E_ARG;
  for (size_t i = 0; i < n; ++i)
    if (rows[i] >= nrows || cols[i] >= npol) return KW_E_ARG;
  std::vector<uint64_t> table;
  if (int rc = patches_table(env->e, policies, npol, &table)) return rc;
  D.patches_ran = true;
  for (uint64_t& v : D.patches_stats) v = 0;
  if (n == 0) {
    if (out->off) out->off[0] = 0;
    return KW_OK;
  }
  RoundsCall call;
  call.t_start = std::chrono::steady_clock::now();
  if (int rc = F.open()) return rc;
  hipStream_t s = F.s;
  if (!D.places) {
    if (int rc = upload_places(b, s)) return rc;
    D.patches_stats[4] = 1;
  }
  if (form == KW_PATCH_RESPONSE && !D.uids) {
    if (int rc = upload_uids(b, s)) return rc;
    D.patches_stats[4] = 1;
  }
  call.side_ms = ms_since(call.t_start);
  const Batch& DB = dev_rows(b);
  PatchesArgs pa{};
  pa.form = (uint32_t)form;
  pa.c.rows = DB.n;
  pa.c.nctr = DB.containers();
  pa.c.ctr_off = D.ctr_off;
  pa.c.capadd_off = D.capadd_off;
  pa.c.capdrop_off = D.capdrop_off;
  pa.c.ctr_flags = D.ctr_flags;
  auto resident = [&](int m) {
    const bool have = ((D.loaded >> m) & 1u) && D.str[m].off && D.str[m].bytes;
    return have ? DigestStr{D.str[m].off, D.str[m].bytes, host_str(DB, m).n()} : DigestStr{nullptr, nullptr, 0};
  };
  pa.c.add = resident(S_CAPADD);
  pa.c.drop = resident(S_CAPDROP);
  if (D.uids) pa.c.uid = DigestStr{D.uid_col.off, D.uid_col.bytes, D.uid_col.n};
  pa.c.ctr_place = D.ctr_place;
  pa.c.req_place = D.req_place;
  ResponsesArgs a{};
  a.cols.c.rows = DB.n;
  call.len = [&pa](const ResponsesArgs& r, hipStream_t st) {
    pa.r = r;
    return launch_patches_len(pa, st);
  };
  call.write = [&pa](const ResponsesArgs& r, hipStream_t st) {
    pa.r = r;
    return launch_patches_write(pa, st);
  };
  call.what = "patches";
  call.stats = D.patches_stats;
  return response_rounds(F, table, a, rows, cols, n, out, call);
}

// The host side over full words [nrows][npol] and the host batch. how 0: format_patch per item; how
// 1: the walk of patches.hpp in the device's rounds, waves and windows.
int debug_patches_words(const kw_env* env, const kw_batch* b, const int32_t* policies, uint32_t npol, const uint32_t* words,
                        uint64_t nrows, const uint64_t* rows, const uint32_t* cols, size_t n, int form, int how, kw_responses* out) {
  if (!out) return KW_E_ARG;
  out->bytes = out->nhost = 0;
  if (!env || !b || npol == 0 || nrows > b->b.n || (nrows && !words) || (how != 0 && how != 1) || !form_ok(form)) return KW_E_ARG;
  if (!responses_out_ok(out, rows, cols, n)) return KW_E_ARG;
  for (size_t i = 0; i < n; ++i)
    if (rows[i] >= nrows || cols[i] >= npol) return KW_E_ARG;
  std::vector<uint64_t> table;
  if (int rc = patches_table(env->e, policies, npol, &table)) return rc;
  if (n == 0) {
    if (out->off) out->off[0] = 0;
    return KW_OK;
  }
  const Batch& B = b->b;
  PatchCtx X;
  X.C = host_patch_cols(B);
  X.S = patch_settings((const uint8_t*)table.data());
  const size_t chunk = (size_t)Knobs::num<KW_MESSAGES_CHUNK>();
  const uint32_t window = msg_window_bytes(Knobs::num<KW_MESSAGES_WINDOW>());
  std::vector<uint8_t> raw(patch_raw_need(window) + 16);
  uint64_t total = 0, nhost = 0;
  std::string text;
  // the lengths, then the text
  std::vector<uint8_t> host_item(n, 0);
  for (size_t i = 0; i < n; ++i) {
    const uint64_t row = rows[i];
    const uint32_t col = cols[i], w = words[row * npol + col];
    out->off[i] = total;
    if (out->words) out->words[i] = w;
    uint32_t st, len = 0;
    if (how == 0) {
      const Status fs = format_patch(env->e, B, row, policies[col], w, form, &text);
      st = fs.ok() ? PATCH_TEXT : PATCH_HOST;
      len = fs.ok() ? (uint32_t)text.size() : 0u;
      if (len && total + len <= out->cap) memcpy(out->text + total, text.data(), len);
    } else {
      st = patch_length(X, row, col, w, (uint32_t)form, &len);
      if (st == PATCH_MISSING) return KW_E_ARG;
    }
    if (st == PATCH_HOST) {
      host_item[i] = 1;
      if (nhost < out->host_cap) out->host[nhost] = i;
      ++nhost;
    }
    total += len;
  }
  out->off[n] = total;
  out->bytes = (size_t)total;
  out->nhost = (size_t)nhost;
  if (total > out->cap || nhost > out->host_cap) return KW_E_NOSPACE;
  if (how == 1) {
    for (size_t i = 0; i < n; ++i) {
      const uint64_t mb = out->off[i];
      const uint32_t len = (uint32_t)(out->off[i + 1] - mb), col = cols[i];
      if (!len || host_item[i]) continue;
      const uint64_t row = rows[i];
      const uint32_t ops = patch_measure(X, row, col);
      const PatchEnvelope e = form == KW_PATCH_RESPONSE ? patch_envelope(X, row) : PatchEnvelope{nullptr, 0, 0, 0};
      // the windows of the item's wave: from the 16-byte boundary at or below the wave's first byte
      const size_t r0 = i / chunk * chunk, i0 = r0 + (i - r0) / kMsgWaveItems * kMsgWaveItems;
      const uint64_t w0 = out->off[i0] & ~(uint64_t)15u;
      for (uint64_t wb = w0 + (mb - w0) / window * window; wb < mb + len; wb += window) {
        uint32_t skip, at, m;
        msg_clip(mb, len, wb, window, &skip, &at, &m);
        if (!m) continue;
        uint8_t* dst = (uint8_t*)out->text + mb + skip;
        if (form == KW_PATCH_RESPONSE) patch_response_window(X, row, col, e, ops, skip, m, dst, raw.data());
        else patch_render_window(X, row, col, skip, m, dst);
      }
    }
  }
  return KW_OK;
}

int debug_patches_stats(const kw_batch* b, uint64_t* out) {
  if (!b || !b->dev || !out || !b->dev->patches_ran) return KW_E_ARG;
  for (int i = 0; i < 5; ++i) out[i] = b->dev->patches_stats[i];
  return KW_OK;
}

}  // namespace kw
