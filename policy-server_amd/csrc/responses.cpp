// responses.cpp — the AdmissionResponse bodies of chosen pairs on a resident pass (include/kwgpu.h):
// kw_batch_responses builds the responses' table from (env, policies), uploads the uid column and
// the container names on first use, and runs the items in the rounds of the messages: the lengths,
// their scan (the messages' scan kernels) and the text are three steps a round, the offsets, the
// words and the host marks come back through a pooled block, the text by direct DMA into page-locked
// memory or through a bounce block (response_rounds, rounds.hpp: kw_batch_patches runs its items
// through the same rounds with its own two launches). The two host renderers of the diagnostic. The
// arithmetic is responses.hpp's, the kernels reports.hip's.
#include "responses.hpp"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "knobs.hpp"
#include "lastpass.hpp"
#include "reports.hpp"
#include "rounds.hpp"
#include "service.hpp"
#include "upload.hpp"

namespace kw {
namespace {

static_assert(sizeof(RspCol) == 28 && sizeof(RspHead) == 24 && sizeof(ResponsesHead) == 32, "responses records");

constexpr size_t kTask = 1u << 16;  // items of one staging task of the host workers

// The responses' table of a pass over `policies` (rsp_build_table); KW_E_ARG for an index outside
// the visible policies. A member's column is the first that holds it.
int responses_table(const Env& E, const int32_t* policies, uint32_t npol, std::vector<uint64_t>* block) {
  if (npol && !policies) return KW_E_ARG;
  std::vector<RspColSource> cols(npol);
  for (uint32_t c = 0; c < npol; ++c) {
    if (policies[c] < 0 || (size_t)policies[c] >= E.nvisible) return KW_E_ARG;
    const PolicyRec& P = E.pol[(size_t)policies[c]];
    RspColSource& s = cols[c];
    s.m.family = P.family;
    s.m.ns = P.lists[0].empty() ? std::string() : P.lists[0][0];
    s.m.message = P.message;
    s.m.init = P.init_message;
    s.m.mandatory = P.lists[1];
    s.m.keys = P.lists[2];
    s.m.regexes = P.lists[3];
    s.id = P.id;
    s.name = P.name;
    s.registered = P.registered;
    s.is_group = P.is_group;
    s.broken = !P.broken_member.empty();
    for (int32_t m : P.members) {
      uint32_t at = kRspAbsent;
      for (uint32_t k = 0; k < npol && at == kRspAbsent; ++k)
        if (policies[k] == m) at = k;
      s.members.push_back(at);
    }
  }
  *block = rsp_build_table(cols);
  return KW_OK;
}

}  // namespace

bool responses_out_ok(const kw_responses* out, const uint64_t* rows, const uint32_t* cols, size_t n) {
  if (!out) return false;
  if (n && (!rows || !cols || !out->off)) return false;
  return !(out->cap && !out->text) && !(out->host_cap && !out->host);
}

// The uid column to the device in device-row order (a split batch: through the upload's row
// permutation), with the zero tail the other pools have.
int upload_uids(kw_batch* kb, hipStream_t s) {
  DeviceBatch& D = *kb->dev;
  const Batch& B = kb->b;
  const StrCol& U = B.uid;
  if (U.n() != B.n) return KW_E_ARG;
  const size_t b_off = round_up((size_t)(B.n + 1) * 4, 256), b_bytes = round_up((size_t)U.off.back() + 32, 256), total = b_off + b_bytes;
  BlockLease h;
  HIPCHK(h.alloc(host_pool(), D.device, total));
  uint32_t* off = (uint32_t*)h.p;
  uint8_t* bytes = (uint8_t*)h.p + b_off;
  memset(bytes, 0, b_bytes);
  if (D.split && D.perm.size() == B.n) {
    off[0] = 0;
    for (uint64_t d = 0; d < B.n; ++d) {
      const uint64_t r = D.perm[d];
      const uint32_t len = U.off[r + 1] - U.off[r];
      memcpy(bytes + off[d], U.bytes.data() + U.off[r], len);
      off[d + 1] = off[d] + len;
    }
  } else {
    memcpy(off, U.off.data(), (size_t)(B.n + 1) * 4);
    if (U.off.back()) memcpy(bytes, U.bytes.data(), U.off.back());
  }
  void* d = nullptr;
  HIPCHK(dev_pool().alloc(D.device, total, &d));
  const hipError_t e1 = hipMemcpyAsync(d, h.p, total, hipMemcpyHostToDevice, s);
  const hipError_t e2 = hipStreamSynchronize(s);  // (the staging block returns to its pool below)
  if (e1 != hipSuccess || e2 != hipSuccess) {
    dev_pool().release(D.device, d, total);
    return KW_E_DEVICE;
  }
  D.uids = (uint8_t*)d;
  D.uids_bytes = total;
  D.uid_col.off = (const uint32_t*)D.uids;
  D.uid_col.bytes = D.uids + b_off;
  D.uid_col.n = B.n;
  D.uid_col.nbytes = U.off.back();
  return KW_OK;
}

int batch_responses(kw_batch* b, const kw_env* env, const int32_t* policies, uint32_t npol, const uint64_t* rows,
                    const uint32_t* cols, size_t n, kw_responses* out) {
  if (!out) return KW_E_ARG;
  out->bytes = out->nhost = 0;
  LastPass F(b, LastPass::kWholeBatch);
  if (!env || !F.ok() || npol != F.npol) return KW_E_ARG;
  const uint64_t nrows = F.rows;
  DeviceBatch& D = *F.dev;
  if (!responses_out_ok(out, rows, cols, n)) return KW_E_ARG;
  for (size_t i = 0; i < n; ++i)
    if (rows[i] >= nrows || cols[i] >= npol) return KW_E_ARG;
  std::vector<uint64_t> table;
  if (int rc = responses_table(env->e, policies, npol, &table)) return rc;
  D.responses_ran = true;
  for (uint64_t& v : D.responses_stats) v = 0;
  if (n == 0) {
    if (out->off) out->off[0] = 0;
    return KW_OK;
  }
  RoundsCall call;
  call.t_start = std::chrono::steady_clock::now();
  if (int rc = F.open()) return rc;
  hipStream_t s = F.s;
  if (!D.names) {
    if (int rc = upload_names(b, s)) return rc;
    D.responses_stats[4] = 1;
  }
  if (!D.uids) {
    if (int rc = upload_uids(b, s)) return rc;
    D.responses_stats[4] = 1;
  }
  call.side_ms = ms_since(call.t_start);
  ResponsesArgs a{};
  a.cols.c = device_cols(b);
  a.cols.name = DigestStr{D.name_col.off, D.name_col.bytes, D.name_col.n};
  a.uid = DigestStr{D.uid_col.off, D.uid_col.bytes, D.uid_col.n};
  call.len = launch_responses_len;
  call.write = launch_responses_write;
  call.what = "responses";
  call.stats = D.responses_stats;
  return response_rounds(F, table, a, rows, cols, n, out, call);
}

int response_rounds(LastPass& F, const std::vector<uint64_t>& table, ResponsesArgs a, const uint64_t* rows, const uint32_t* cols,
                    size_t n, kw_responses* out, const RoundsCall& call) {
  DeviceBatch& D = *F.dev;
  hipStream_t s = F.s;
  const bool dbg = Knobs::on<KW_BULK_DEBUG>();
  const auto t_start = call.t_start;
  const double side_ms = call.side_ms;
  const size_t chunk = (size_t)Knobs::num<KW_MESSAGES_CHUNK>(), m_max = std::min(chunk, n);
  const uint32_t window = msg_window_bytes(Knobs::num<KW_MESSAGES_WINDOW>());
  if (D.split) D.device_rows();

  // in: [device rows][cols][table]; out: [off][words][marks][head]; the device's lengths and the scan's tile sums beside them
  const size_t b_idx = round_up(m_max * 4, 256), b_set = round_up(table.size() * 8, 256), b_in = 2 * b_idx + b_set;
  const size_t b_off = round_up((m_max + 1) * 8, 256), b_words = round_up(m_max * 4, 256), b_mark = round_up(m_max, 256),
               b_out = b_off + b_words + b_mark + round_up(sizeof(ResponsesHead), 256);
  BlockLease &din = F.lease(), &dout = F.lease(), &dlen = F.lease(), &dtext = F.lease(), &hin = F.lease(), &hout = F.lease(),
             &bounce = F.lease();
  HIPCHK(hin.alloc(host_pool(), D.device, b_in));
  HIPCHK(hout.alloc(host_pool(), D.device, b_out));
  HIPCHK(din.alloc(dev_pool(), D.device, b_in));
  HIPCHK(dout.alloc(dev_pool(), D.device, b_out));
  HIPCHK(dlen.alloc(dev_pool(), D.device, b_idx + round_up((m_max / kMsgScanTile + 1) * 8, 256)));
  uint8_t *hi = (uint8_t*)hin.p, *ho = (uint8_t*)hout.p, *di = (uint8_t*)din.p, *dov = (uint8_t*)dout.p;
  memset(hi + 2 * b_idx, 0, b_set);
  memcpy(hi + 2 * b_idx, table.data(), table.size() * 8);
  HIPCHK(hipMemcpyAsync(di + 2 * b_idx, hi + 2 * b_idx, b_set, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(dov + b_off + b_words + b_mark, 0, sizeof(ResponsesHead), s));

  a.words = D.verdicts;
  a.settings = di + 2 * b_idx;
  a.drow = (const uint32_t*)di;
  a.col = (const uint32_t*)(di + b_idx);
  a.len = (uint32_t*)dlen.p;
  a.out_words = out->words ? (uint32_t*)(dov + b_off) : nullptr;
  a.mark = dov + b_off + b_words;
  a.off = (const uint64_t*)dov;
  a.head = (ResponsesHead*)(dov + b_off + b_words + b_mark);
  a.npol = F.npol;
  a.window = window;
  MessagesArgs sc{};  // what the messages' scan kernels read of their arguments
  sc.len = a.len;
  sc.off = (uint64_t*)dov;
  sc.sums = (uint64_t*)((uint8_t*)dlen.p + b_idx);

  const bool direct = out->cap && page_locked(out->text);
  StreamTimer t_len(dbg), t_scan(dbg), t_write(dbg), t_back(dbg);
  double len_ms = 0, scan_ms = 0, write_ms = 0, back_ms = 0, text_ms = 0;
  uint64_t total = 0, nhost = 0, rounds = 0;
  for (size_t r0 = 0; r0 < n; r0 += chunk, ++rounds) {
    const size_t m = std::min(chunk, n - r0);
    uint32_t *hr = (uint32_t*)hi, *hc = (uint32_t*)(hi + b_idx);
    HostWorkers::get().run((m + kTask - 1) / kTask, [&](size_t q) {
      for (size_t i = q * kTask, e = std::min(m, (q + 1) * kTask); i < e; ++i) {
        hr[i] = (uint32_t)(D.split ? D.inv_perm[rows[r0 + i]] : rows[r0 + i]);
        hc[i] = cols[r0 + i];
      }
    });
    HIPCHK(hipMemcpyAsync(di, hi, m * 4, hipMemcpyHostToDevice, s));  // (the round's items, not the block)
    HIPCHK(hipMemcpyAsync(di + b_idx, hi + b_idx, m * 4, hipMemcpyHostToDevice, s));
    a.n = sc.n = (uint32_t)m;
    sc.base = total;
    t_len.start(s);
    HIPCHK(call.len(a, s));
    t_len.stop(s);
    t_scan.start(s);
    HIPCHK(launch_messages_scan(sc, s));
    t_scan.stop(s);
    t_back.start(s);
    // what the round wrote, sized by its items: the offsets, the words when asked for, the marks, the head
    HIPCHK(hipMemcpyAsync(ho, dov, (m + 1) * 8, hipMemcpyDeviceToHost, s));
    if (out->words) HIPCHK(hipMemcpyAsync(ho + b_off, dov + b_off, m * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ho + b_off + b_words, dov + b_off + b_words, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ho + b_off + b_words + b_mark, dov + b_off + b_words + b_mark, sizeof(ResponsesHead), hipMemcpyDeviceToHost, s));
    t_back.stop(s);
    HIPCHK(hipStreamSynchronize(s));
    len_ms += t_len.ms(), scan_ms += t_scan.ms(), back_ms += t_back.ms();
    const ResponsesHead head = *(const ResponsesHead*)(ho + b_off + b_words + b_mark);
    if (head.missing) return KW_E_ARG;  // a response quotes a string column that is not resident
    const uint64_t* off = (const uint64_t*)ho;
    if (off[0] != total) return KW_E_ENGINE;
    parallel_copy(out->off + r0, off, (m + 1) * 8);
    if (out->words) parallel_copy(out->words + r0, ho + b_off, m * 4);
    const uint8_t* mark = ho + b_off + b_words;
    for (size_t i = 0; i < m;) {
      uint64_t eight = 0;
      if (i + 8 <= m) {
        memcpy(&eight, mark + i, 8);
        if (!eight) {
          i += 8;
          continue;
        }
      }
      for (const size_t e = std::min(m, i + 8); i < e; ++i)
        if (mark[i]) {
          if (nhost < out->host_cap) out->host[nhost] = r0 + i;
          ++nhost;
        }
    }
    const uint64_t end = off[m];
    if (end > total && end <= out->cap) {  // (past cap only the lengths run: text is then unspecified)
      a.text_base = total & ~(uint64_t)15u;
      const size_t b_text = (size_t)(end - a.text_base) + 16;
      HIPCHK(dtext.alloc(dev_pool(), D.device, b_text));
      a.text = (uint8_t*)dtext.p;
      t_write.start(s);
      HIPCHK(call.write(a, s));
      t_write.stop(s);
      const uint8_t* src = a.text + (total - a.text_base);
      const size_t bytes = (size_t)(end - total);
      const auto t_text = std::chrono::steady_clock::now();
      if (direct) {
        HIPCHK(hipMemcpyAsync(out->text + total, src, bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
      } else if (int rc = bounce_read(bounce, D.device, s, out->text + total, src, bytes)) {
        return rc;
      }
      write_ms += t_write.ms();
      text_ms += ms_since(t_text);
    }
    total = end;
  }
  out->bytes = (size_t)total;
  out->nhost = (size_t)nhost;
  // the counters of the launches
  HIPCHK(hipMemcpyAsync(ho, a.head, sizeof(ResponsesHead), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const ResponsesHead head = *(const ResponsesHead*)ho;
  call.stats[0] = rounds;
  call.stats[1] = head.windows;
  call.stats[2] = head.spanning;
  call.stats[3] = nhost;
  call.stats[5] = head.escaped;
  const bool fits = total <= out->cap && nhost <= out->host_cap;
  if (dbg)
    fprintf(stderr, "[kw %s] %zu items, %llu bytes, %llu for the host, %llu rounds, window %u%s: side columns %.3f ms, len %.3f ms "
            "scan %.3f ms write %.3f ms on the device (by events), offsets read-back %.3f ms (by events), text read-back %.3f ms (%s), "
            "the call %.3f ms\n",
            call.what, n, (unsigned long long)total, (unsigned long long)nhost, (unsigned long long)rounds, window, fits ? "" : " (more than cap)",
            side_ms, len_ms, scan_ms, write_ms, back_ms, text_ms, direct ? "direct" : "bounce", ms_since(t_start));
  return fits ? KW_OK : KW_E_NOSPACE;
}

// The host side over full words [nrows][npol] and the host batch. how 0: format_response per item;
// how 1: the part renderer over the host columns.
int debug_responses_words(const kw_env* env, const kw_batch* b, const int32_t* policies, uint32_t npol, const uint32_t* words,
                          uint64_t nrows, const uint64_t* rows, const uint32_t* cols, size_t n, int how, kw_responses* out) {
  if (!out) return KW_E_ARG;
  out->bytes = out->nhost = 0;
  if (!env || !b || npol == 0 || nrows > b->b.n || (nrows && !words) || (how != 0 && how != 1)) return KW_E_ARG;
  if (!responses_out_ok(out, rows, cols, n)) return KW_E_ARG;
  for (size_t i = 0; i < n; ++i)
    if (rows[i] >= nrows || cols[i] >= npol) return KW_E_ARG;
  std::vector<uint64_t> table;
  if (int rc = responses_table(env->e, policies, npol, &table)) return rc;
  if (n == 0) {
    if (out->off) out->off[0] = 0;
    return KW_OK;
  }
  const Batch& B = b->b;
  RspCtx X;
  X.C.c = host_cols(B);
  X.C.name = DigestStr{B.ctr_name.off.data(), B.ctr_name.bytes.data(), B.ctr_name.n()};
  X.uid = DigestStr{B.uid.off.data(), B.uid.bytes.data(), B.uid.n()};
  X.S = rsp_settings((const uint8_t*)table.data());
  X.words = words;
  X.npol = npol;
  uint64_t total = 0, nhost = 0;
  std::string text;
  std::vector<uint32_t> mv;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t row = rows[i];
    const uint32_t col = cols[i], w = words[row * npol + col];
    out->off[i] = total;
    if (out->words) out->words[i] = w;
    RspItem it;
    uint32_t st = rsp_item(X.S, col, w, &it);
    size_t len = 0;
    if (st == RSP_TEXT && how == 0) {
      // the members' words of the same row, settings order; a cause the rules leave to the host
      const RspCol& c = X.S.col[col];
      mv.assign(std::max<size_t>(c.nmem, 1), 0u);
      for (uint32_t s = 0; s < c.nmem; ++s) {
        const uint32_t mc = X.S.mem[c.mem_at + s];
        if (mc != kRspAbsent) mv[s] = words[row * npol + mc];
        if (it.form == RF_GROUP && s < 16u && ((it.mask >> s) & 1u) && !rsp_member_mutated(mv[s]) && rsp_member_host(mv[s])) st = RSP_HOST;
      }
      if (st == RSP_TEXT) {
        const Status fs = format_response(env->e, B, row, policies[col], w, mv.data(), &text, nullptr, 0, 0);
        if (!fs.ok()) st = RSP_HOST;
        else len = text.size();
      }
      if (len && total + len <= out->cap) memcpy(out->text + total, text.data(), len);
    } else if (st == RSP_TEXT) {
      uint32_t l = 0, nesc = 0;
      st = rsp_measure(X, row, col, w, it, &l, &nesc);
      if (st == RSP_MISSING) return KW_E_ARG;
      len = l;
      if (len && total + len <= out->cap) rsp_render_window(X, row, col, w, it, 0, l, (uint8_t*)out->text + total);
    }
    if (st == RSP_HOST) {
      len = 0;
      if (nhost < out->host_cap) out->host[nhost] = i;
      ++nhost;
    }
    total += len;
  }
  out->off[n] = total;
  out->bytes = (size_t)total;
  out->nhost = (size_t)nhost;
  return total <= out->cap && nhost <= out->host_cap ? KW_OK : KW_E_NOSPACE;
}

int debug_responses_stats(const kw_batch* b, uint64_t* out) {
  if (!b || !b->dev || !out || !b->dev->responses_ran) return KW_E_ARG;
  for (int i = 0; i < 6; ++i) out[i] = b->dev->responses_stats[i];
  return KW_OK;
}

}  // namespace kw
