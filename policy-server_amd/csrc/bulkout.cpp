// bulkout.cpp — the three output forms of a bulk pass; what each step does and in what order: bulkout.hpp.
#include "bulkout.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "reports.hpp"
#include "knobs.hpp"
#include "packed.hpp"

namespace kw {

// ---- the words ----
int WordsOut::setup(const BulkCtx& c, uint64_t max_rows) {
  if (!c.pinned)
    for (BlockLease& b : c.blk.bounce) HIPCHK(b.alloc(host_pool(), c.device, (size_t)max_rows * c.npol * 4));
  return KW_OK;
}

int WordsOut::copies(const BulkCtx& c, uint64_t k) {
  const uint64_t r0 = c.rb[k], r1 = c.rb[k + 1];
  uint32_t* dst = c.pinned ? out + r0 * c.npol : (uint32_t*)c.blk.bounce[k & 1].p;
  HIPCHK(hipMemcpyAsync(dst, c.words + r0 * c.npol, (size_t)(r1 - r0) * c.npol * 4, hipMemcpyDeviceToHost, c.s_out));
  return KW_OK;
}

int WordsOut::landed(const BulkCtx& c, uint64_t k) {
  const auto t0 = clk::now();
  if (c.pinned) return KW_OK;
  HIPCHK(hipEventSynchronize(c.ev[3 * k + 2]));
  const uint64_t r0 = c.rb[k], r1 = c.rb[k + 1];
  parallel_copy_segs({{out + r0 * c.npol, c.blk.bounce[k & 1].p, (size_t)(r1 - r0) * c.npol * 4}});
  c.t.out += since(t0);
  return KW_OK;
}

// ---- planes ----
int PlanesOut::carve(const BulkCtx& c, const std::vector<size_t>& bytes, uint8_t** at) {
  size_t total = 0;
  for (size_t b : bytes) total += up(b);
  HIPCHK(c.blk.dfix.alloc(dev_pool(), c.device, total));
  uint8_t* d = (uint8_t*)c.blk.dfix.p;
  for (size_t b : bytes) *at++ = d, d += up(b);
  return KW_OK;
}

int PlanesOut::copy_planes(const BulkCtx& c, uint64_t k) const {
  const uint64_t r0 = c.rb[k], r1 = c.rb[k + 1];
  if (h_planes && r1 > r0)
    HIPCHK(hipMemcpyAsync(c.pinned ? (void*)(h_planes + 2 * r0 * G) : c.blk.bounce[k & 1].p, d_planes + 2 * r0 * G,
                          (size_t)(r1 - r0) * G * 16, hipMemcpyDeviceToHost, c.s_out));
  return KW_OK;
}

CopySeg PlanesOut::planes_seg(const BulkCtx& c, uint64_t k) const {
  return {h_planes + 2 * c.rb[k] * G, c.blk.bounce[k & 1].p, (size_t)(c.rb[k + 1] - c.rb[k]) * G * 16};
}

// ---- the packed form ----
int PackedOut::setup(const BulkCtx& c, uint64_t max_rows) {
  const uint64_t items = packed_items(c.rows, c.npol);
  G = packed_groups(c.npol);
  const size_t b_dict = (size_t)c.npol * 12, b_tot = up((c.K + 1) * 4);
  uint8_t* d[6];
  if (int rc = carve(c, {(size_t)items * 16, b_dict, b_tot, ((size_t)max_rows * G / kScanBlock + 1) * 4,
                         (size_t)(c.rows + 1) * 4, (size_t)items * 4}, d))
    return rc;
  d_planes = (uint64_t*)d[0], d_dict = (uint32_t*)d[1], d_tot = (uint32_t*)d[2];
  d_bsum = (uint32_t*)d[3], d_off = (uint32_t*)d[4], d_ibase = (uint32_t*)d[5];
  slot_words = (size_t)max_rows * c.npol;
  HIPCHK(c.blk.dexc.alloc(dev_pool(), c.device, kXRing * slot_words * 4));
  HIPCHK(c.blk.hfix.alloc(host_pool(), c.device, b_tot + up(b_dict)));
  h_tot = (volatile uint32_t*)c.blk.hfix.p;
  for (uint64_t k = 0; k <= c.K; ++k) h_tot[k] = 0;
  uint32_t* h_dict = (uint32_t*)((uint8_t*)c.blk.hfix.p + b_tot);
  memcpy(h_dict, pk->dict, b_dict);
  off_at = up((size_t)max_rows * G * 16);
  if (!c.pinned) {
    for (BlockLease& b : c.blk.bounce) HIPCHK(b.alloc(host_pool(), c.device, off_at + (size_t)(max_rows + 1) * 4));
    for (BlockLease& b : c.blk.xb) HIPCHK(b.alloc(host_pool(), c.device, std::max<size_t>(slot_words, 1) * 4));
  }
  xissued.assign(c.K, 0);
  HIPCHK(hipMemcpyAsync(d_dict, h_dict, b_dict, hipMemcpyHostToDevice, c.sc));
  HIPCHK(hipMemsetAsync(d_tot, 0, 4, c.sc));
  return KW_OK;
}

int PackedOut::reduce(const BulkCtx& c, uint64_t k) {
  const uint64_t r0 = c.rb[k], r1 = c.rb[k + 1];
  if (k >= kXRing && xissued[k - kXRing]) HIPCHK(hipStreamWaitEvent(c.sc, c.ev[3 * c.K + k - kXRing], 0));  // ring slot free
  if (r1 == r0) {  // (no rows: the total passes through)
    HIPCHK(hipMemcpyAsync(d_tot + k + 1, d_tot + k, 4, hipMemcpyDeviceToDevice, c.sc));
    return KW_OK;
  }
  PackArgs a;
  a.words = c.words + r0 * c.npol;
  a.dict = d_dict;
  a.planes = d_planes + 2 * r0 * G;
  a.ibase = d_ibase + r0 * G;
  a.exc_off = d_off + r0;
  a.bsum = d_bsum;
  a.tot = d_tot + k;
  a.exc = (uint32_t*)c.blk.dexc.p + (k % kXRing) * slot_words;
  a.exc_cap = (uint32_t)std::min<uint64_t>((r1 - r0) * c.npol, slot_words);
  a.npol = c.npol;
  a.G = G;
  a.nitems = (uint32_t)((r1 - r0) * G);
  HIPCHK(launch_pack(a, c.sc));
  return KW_OK;
}

int PackedOut::copies(const BulkCtx& c, uint64_t k) {
  const uint64_t r0 = c.rb[k], noff = c.rb[k + 1] - r0 + (k + 1 == c.K ? 1 : 0);  // (the last chunk brings the final total)
  if (int rc = copy_planes(c, k)) return rc;
  if (noff)
    HIPCHK(hipMemcpyAsync(c.pinned ? (void*)(pk->exc_off + r0) : (void*)((uint8_t*)c.blk.bounce[k & 1].p + off_at), d_off + r0,
                          (size_t)noff * 4, hipMemcpyDeviceToHost, c.s_out));
  HIPCHK(hipMemcpyAsync((void*)(h_tot + k + 1), d_tot + k + 1, 4, hipMemcpyDeviceToHost, c.s_out));
  return KW_OK;
}

int PackedOut::copy_out_exc(const BulkCtx& c, uint64_t k) {
  if (c.pinned || !xissued[k]) return KW_OK;
  HIPCHK(hipEventSynchronize(c.ev[3 * c.K + k]));
  parallel_copy_segs({{pk->exc + h_tot[k], c.blk.xb[k % 3].p, (size_t)(h_tot[k + 1] - h_tot[k]) * 4}});
  return KW_OK;
}

int PackedOut::landed(const BulkCtx& c, uint64_t k) {
  const auto t0 = clk::now();
  HIPCHK(hipEventSynchronize(c.ev[3 * k + 2]));
  if (!c.pinned) {
    const uint64_t r0 = c.rb[k], noff = c.rb[k + 1] - r0 + (k + 1 == c.K ? 1 : 0);
    parallel_copy_segs({planes_seg(c, k), {pk->exc_off + r0, (const uint8_t*)c.blk.bounce[k & 1].p + off_at, (size_t)noff * 4}});
    if (k >= 2)  // (two steps behind its read-back: the host does not wait for a copy just queued)
      if (int rc = copy_out_exc(c, k - 2)) return rc;
  }
  const uint32_t t_lo = h_tot[k], t_hi = h_tot[k + 1];
  if (t_hi > pk->exc_cap) nospace = true;  // (the pass goes on and counts)
  if (!nospace && t_hi > t_lo) {
    const uint32_t* src = (const uint32_t*)c.blk.dexc.p + (k % kXRing) * slot_words;
    HIPCHK(hipMemcpyAsync(c.pinned ? (void*)(pk->exc + t_lo) : c.blk.xb[k % 3].p, src, (size_t)(t_hi - t_lo) * 4,
                          hipMemcpyDeviceToHost, c.s_out));
    HIPCHK(hipEventRecord(c.ev[3 * c.K + k], c.s_out));
    xissued[k] = 1;
  }
  c.t.out += since(t0);
  return KW_OK;
}

int PackedOut::end(const BulkCtx& c) {
  if (const uint64_t K = c.K) {
    if (int rc = landed(c, K - 1)) return rc;
    if (K >= 2)
      if (int rc = copy_out_exc(c, K - 2)) return rc;
    if (int rc = copy_out_exc(c, K - 1)) return rc;
    if (xissued[K - 1]) HIPCHK(hipEventSynchronize(c.ev[3 * K + K - 1]));
  }
  pk->exc_count = c.K ? h_tot[c.K] : 0;
  if (Knobs::on<KW_BULK_DEBUG>())
    fprintf(stderr, "[kw bulk] packed: %llu exception words of %llu (capacity %llu), %.1f B per row read back\n",
            (unsigned long long)pk->exc_count, (unsigned long long)(c.rows * c.npol), (unsigned long long)pk->exc_cap,
            c.rows ? ((double)pk->exc_count * 4 + (double)c.rows * (G * 16 + 4)) / (double)c.rows : 0.0);
  return nospace ? KW_E_NOSPACE : KW_OK;
}

// ---- the summary form ----
int SummaryOut::setup(const BulkCtx& c, uint64_t max_rows) {
  G = packed_groups(c.npol);
  const size_t b_tot = summary_col_words(c.npol) * 8;
  uint8_t* d[3];
  if (int rc = carve(c, {h_planes ? (size_t)c.rows * G * 16 : 0, b_tot, summary_part_bytes(max_rows, c.npol)}, d)) return rc;
  d_planes = (uint64_t*)d[0], d_tot = (uint64_t*)d[1], d_part = (uint32_t*)d[2];
  HIPCHK(c.blk.hfix.alloc(host_pool(), c.device, up(b_tot)));
  if (!c.pinned && h_planes)
    for (BlockLease& b : c.blk.bounce) HIPCHK(b.alloc(host_pool(), c.device, std::max<size_t>((size_t)max_rows * G * 16, 16)));
  HIPCHK(hipMemsetAsync(d_tot, 0, b_tot, c.sc));
  return KW_OK;
}

int SummaryOut::reduce(const BulkCtx& c, uint64_t k) {
  const uint64_t r0 = c.rb[k], r1 = c.rb[k + 1];
  SumArgs a;
  a.words = c.words + r0 * c.npol;
  a.planes = h_planes ? d_planes + 2 * r0 * G : nullptr;
  a.part = d_part;
  a.tot = d_tot;
  a.rows = r1 - r0;
  a.npol = c.npol;
  HIPCHK(launch_summary(a, c.sc));
  return KW_OK;
}

int SummaryOut::landed(const BulkCtx& c, uint64_t k) {
  if (c.pinned || !h_planes) return KW_OK;  // (KW_BULK_DIRECT=0 clears `pinned` for a counters-only pass too)
  const auto t0 = clk::now();
  HIPCHK(hipEventSynchronize(c.ev[3 * k + 2]));
  parallel_copy_segs({planes_seg(c, k)});
  c.t.out += since(t0);
  return KW_OK;
}

int SummaryOut::end(const BulkCtx& c) {
  if (c.K)
    if (int rc = landed(c, c.K - 1)) return rc;
  const size_t b_tot = summary_col_words(c.npol) * 8;
  HIPCHK(hipMemcpyAsync(c.blk.hfix.p, d_tot, b_tot, hipMemcpyDeviceToHost, c.s_out));
  HIPCHK(hipStreamSynchronize(c.s_out));
  memcpy(sm->col, c.blk.hfix.p, b_tot);
  return KW_OK;
}

}  // namespace kw
