// summary.cpp — the summary form's entries on a resident pass (include/kwgpu.h): kw_batch_summary
// reduces the last pass's verdict words on the device and reads back the counters and the planes;
// kw_batch_verdict_rows gathers the words of chosen rows, sized by kw_batch_last_pass; the
// host-reducer diagnostic. The arithmetic is summary.hpp's, the kernels reports.hip's, the bulk
// pass bulk.cpp's, its summary form bulkout.cpp's.
#include "summary.hpp"

#include <cstdio>
#include <cstring>

#include "knobs.hpp"
#include "lastpass.hpp"
#include "reports.hpp"
#include "upload.hpp"

namespace kw {
namespace {

int batch_summary(kw_batch* b, kw_summary* out) {
  LastPass F(b, LastPass::kAnyPass);
  if (!out || !out->col || !F.ok()) return KW_E_ARG;
  const uint64_t rows = F.rows;
  const uint32_t npol = F.npol;
  if (out->rows != rows || out->npol != npol) return KW_E_ARG;
  DeviceBatch& D = *F.dev;
  if (int rc = F.open()) return rc;
  hipStream_t s = F.s;
  const uint32_t G = packed_groups(npol);
  const size_t b_tot = summary_col_words(npol) * 8, b_planes = (size_t)rows * G * 16;
  const bool planes = out->planes && rows;
  BlockLease &dtot = F.lease(), &dpart = F.lease(), &dplanes = F.lease(), &htot = F.lease(), &bounce = F.lease();
  HIPCHK(dtot.alloc(dev_pool(), D.device, b_tot));
  HIPCHK(htot.alloc(host_pool(), D.device, b_tot));
  HIPCHK(dpart.alloc(dev_pool(), D.device, std::max<size_t>(summary_part_bytes(rows, npol), 256)));
  if (planes) HIPCHK(dplanes.alloc(dev_pool(), D.device, b_planes));
  StreamTimer timer(Knobs::on<KW_BULK_DEBUG>());
  timer.start(s);
  HIPCHK(hipMemsetAsync(dtot.p, 0, b_tot, s));
  SumArgs a;
  a.words = D.verdicts;
  a.planes = planes ? (uint64_t*)dplanes.p : nullptr;
  a.part = (uint32_t*)dpart.p;
  a.tot = (uint64_t*)dtot.p;
  a.rows = rows;
  a.npol = npol;
  HIPCHK(launch_summary(a, s));
  timer.stop(s);
  HIPCHK(hipMemcpyAsync(htot.p, dtot.p, b_tot, hipMemcpyDeviceToHost, s));
  if (planes && !D.split && page_locked(out->planes)) {
    HIPCHK(hipMemcpyAsync(out->planes, dplanes.p, b_planes, hipMemcpyDeviceToHost, s));
  } else if (planes && !D.split) {
    if (int rc = bounce_read(bounce, D.device, s, out->planes, dplanes.p, b_planes)) return rc;
  } else if (planes) {
    // a split batch holds its rows in device order: through the bounce block by whole rows, each
    // row's plane words to its batch row (read_verdicts does the same for words)
    const size_t rb = (size_t)G * 16, per = std::max<size_t>(1, kBounce / rb);
    HIPCHK(bounce.alloc(host_pool(), D.device, std::min(kBounce, std::max<size_t>(b_planes, rb))));
    for (uint64_t d0 = 0; d0 < rows; d0 += per) {
      const uint64_t d1 = std::min<uint64_t>(rows, d0 + per);
      HIPCHK(hipMemcpyAsync(bounce.p, (const uint8_t*)dplanes.p + d0 * rb, (d1 - d0) * rb, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      const uint8_t* src = (const uint8_t*)bounce.p;
      HostWorkers::get().run((size_t)((d1 - d0 + 4095) / 4096), [&](size_t q) {
        for (uint64_t d = d0 + q * 4096, e = std::min(d1, d0 + (q + 1) * 4096); d < e; ++d)
          memcpy((uint8_t*)out->planes + D.perm[d] * rb, src + (d - d0) * rb, rb);
      });
    }
  }
  HIPCHK(hipStreamSynchronize(s));
  if (timer.on)
    fprintf(stderr, "[kw summary] %llu rows x %u%s: zero + reduce %.3f ms on the device\n", (unsigned long long)rows, npol,
            planes ? ", planes" : "", timer.ms());
  memcpy(out->col, htot.p, b_tot);
  return KW_OK;
}

int batch_verdict_rows(kw_batch* b, const uint64_t* rows, size_t n, uint32_t* out) {
  LastPass F(b, LastPass::kAnyPass);
  if (!F.ok() || (n && (!rows || !out))) return KW_E_ARG;
  const uint64_t nrows = F.rows;
  const uint32_t rw = F.npol;
  for (size_t i = 0; i < n; ++i)
    if (rows[i] >= nrows) return KW_E_ARG;
  if (n == 0) return KW_OK;
  DeviceBatch& D = *F.dev;
  if (int rc = F.open()) return rc;
  hipStream_t s = F.s;
  if (D.split) D.device_rows();
  const size_t b_idx = n * 8, b_out = n * (size_t)rw * 4;
  BlockLease &didx = F.lease(), &dout = F.lease(), &hidx = F.lease(), &hout = F.lease();
  HIPCHK(hidx.alloc(host_pool(), D.device, b_idx));
  HIPCHK(hout.alloc(host_pool(), D.device, b_out));
  HIPCHK(didx.alloc(dev_pool(), D.device, b_idx));
  HIPCHK(dout.alloc(dev_pool(), D.device, b_out));
  uint64_t* idx = (uint64_t*)hidx.p;
  for (size_t i = 0; i < n; ++i) idx[i] = D.split ? D.inv_perm[rows[i]] : rows[i];
  HIPCHK(hipMemcpyAsync(didx.p, hidx.p, b_idx, hipMemcpyHostToDevice, s));
  GatherArgs g;
  g.words = D.verdicts;
  g.rows = (const uint64_t*)didx.p;
  g.out = (uint32_t*)dout.p;
  g.n = n;
  g.row_words = rw;
  HIPCHK(launch_gather_rows(g, s));
  HIPCHK(hipMemcpyAsync(hout.p, dout.p, b_out, hipMemcpyDeviceToHost, s));
  if (int rc = load_side_data(b, s)) return rc;  // (synchronises s)
  memcpy(out, hout.p, b_out);
  return KW_OK;
}

}  // namespace
}  // namespace kw

extern "C" {

int kw_batch_summary(kw_batch* b, kw_summary* out) { return kw::batch_summary(b, out); }

int kw_validate_host_summary(const kw_env* env, kw_batch* b, const int32_t* policies, uint32_t npol, int origin, int device,
                             kw_summary* out, uint32_t chunk_rows) {
  return kw::validate_host_summary(env, b, policies, npol, origin, device, out, chunk_rows);
}

int kw_batch_verdict_rows(kw_batch* b, const uint64_t* rows, size_t n, uint32_t* out) {
  return kw::batch_verdict_rows(b, rows, n, out);
}

int kw_debug_summarize_words(const uint32_t* words, uint64_t rows, uint32_t npol, kw_summary* out) {
  if (!out || out->rows != rows || out->npol != npol) return KW_E_ARG;
  return kw::summary_reduce(words, out);
}

}  // extern "C"
