// bulkout.hpp — the output forms of a bulk pass (bulkout.cpp): what becomes of a chunk's verdict
// words once its kernels are queued. The pass (bulk.cpp, whose head gives the per-chunk contract)
// drives one form through reduce / copies / landed per chunk and end() after the last. A form owns
// its state but no lease: its blocks are members of the pass's Res (OutBlocks), which drains the
// three streams before any block returns to its pool.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <vector>

#include "pass.hpp"
#include "pools.hpp"
#include "summary.hpp"
#include "upload.hpp"

namespace kw {

using clk = std::chrono::steady_clock;
inline double since(clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); }

// diagnostics (KW_BULK_DEBUG=1): host wall time of each stage in ms, printed at the end
struct BulkTimes {
  double layout = 0, plan = 0, prep = 0, desc = 0, fill = 0, enq = 0, out = 0, first = -1, wait = 0;
};

// The forms' blocks, members of Res. bounce: a pageable output's chunks land in block k & 1. dfix:
// the form's device arrays (one block, carved); hfix: its pinned host words. Packed form only: dexc,
// the device exception ring, and xb, a pageable output's exception blocks.
struct OutBlocks {
  BlockLease bounce[2], dfix, dexc, hfix, xb[3];
};

// What a form needs from the pass, made anew for every call.
struct BulkCtx {
  OutBlocks& blk;
  hipStream_t sc, s_out;
  const EventLease& ev;   // chunk k: ev[3k+1] evaluated, ev[3k+2] read back; a form's own from ev[3K] on
  const uint32_t* words;  // the batch's verdict buffer [rows][npol]
  int device;
  uint32_t npol;
  uint64_t rows, K;
  const std::vector<uint64_t>& rb;  // chunk k: rows [rb[k], rb[k+1])
  bool pinned;                      // direct() and KW_BULK_DIRECT: the copies go straight to the caller's arrays
  BulkTimes& t;                     // (t.out: the host's copy-out time)
};

struct BulkOut {
  virtual ~BulkOut() = default;
  virtual bool direct() const = 0;  // every array the form DMA's into is page-locked
  virtual uint32_t events_per_chunk() const { return 3; }
  virtual bool tolerates(int) const { return false; }  // an error after which the pass still stands
  // An unchunked pass: gone through in row slabs by the chunks' steps, or read back by whole().
  virtual bool in_slabs() const { return true; }
  virtual int whole(kw_batch*) { return KW_E_ARG; }
  virtual void empty() {}  // the result of a pass in slabs without rows (K == 0)
  // The blocks for chunks of at most max_rows rows; the form's device state initialised on sc.
  virtual int setup(const BulkCtx& c, uint64_t max_rows) = 0;
  virtual int reduce(const BulkCtx&, uint64_t) { return KW_OK; }  // sc: the form's kernels over chunk k's rows
  virtual int copies(const BulkCtx& c, uint64_t k) = 0;           // s_out: chunk k's D2H copies, inside the pass's event bracket
  virtual int landed(const BulkCtx& c, uint64_t k) = 0;           // the host side of chunk k once it is back
  virtual int end(const BulkCtx& c) = 0;                          // after the last chunk: landed(K-1), what closes the form
};

// kw_validate_host: the words themselves.
//   copies(k)     D2H of the chunk's verdicts into the caller's pinned buffer or bounce block k & 1
//   landed(k-1)   (pageable output) host waits ev[3(k-1)+2], copies bounce block (k-1) & 1 out
//                 (bounce[k & 1] was last read by chunk k-2's copy-out)
// An unchunked pass is read back whole (read_verdicts).
struct WordsOut final : BulkOut {
  uint32_t* out;
  size_t count;
  WordsOut(uint32_t* o, size_t n) : out(o), count(n) {}
  bool direct() const override { return page_locked(out); }
  bool in_slabs() const override { return false; }
  int whole(kw_batch* kb) override { return read_verdicts(kb, out, count); }
  int setup(const BulkCtx& c, uint64_t max_rows) override;
  int copies(const BulkCtx& c, uint64_t k) override;
  int landed(const BulkCtx& c, uint64_t k) override;
  int end(const BulkCtx& c) override { return c.K ? landed(c, c.K - 1) : KW_OK; }
};

// What the packed and the summary form share: two u64 plane words per (row, 64-column group), written
// by the form's kernels into a device array over all rows and read back chunk by chunk.
struct PlanesOut : BulkOut {
  uint64_t* const h_planes;  // the caller's array (null: a summary without planes)
  uint32_t G = 1;
  uint64_t* d_planes = nullptr;
  explicit PlanesOut(uint64_t* h) : h_planes(h) {}
  static size_t up(size_t b) { return (b + 255) & ~(size_t)255; }
  // bytes.size() arrays of bytes[i] bytes, each rounded up to 256, in one device block (blk.dfix); at[i]: array i.
  static int carve(const BulkCtx& c, const std::vector<size_t>& bytes, uint8_t** at);
  int copy_planes(const BulkCtx& c, uint64_t k) const;  // s_out: the chunk's planes to the caller's array or bounce k & 1
  CopySeg planes_seg(const BulkCtx& c, uint64_t k) const;  // bounce k & 1 -> the caller's array
};

// kw_validate_host_packed (packed.hpp): the device packs each chunk's words into planes, per-row
// offsets and exception words. Chunk k also owns ev[3K+k] (its exception words read back) and slot
// k % kXRing of the device exception ring. The dictionary goes up and the running total is zeroed on
// sc ahead of the first chunk.
//   reduce(k)     sc: waits ev[3K+k-kXRing] (the ring slot's previous read-back, where one was
//                 issued), the five pack kernels over the chunk's rows; the scan is seeded with the
//                 device-resident total chunk k-1's scan left (a chunk of no rows: a 4-byte D2D copy
//                 passes the total through)
//   copies(k)     D2H of the chunk's planes, offsets and its 4-byte running total (into the caller's
//                 pinned arrays or bounce block k & 1; the total into a pinned word per chunk)
//   landed(k-1)   host waits ev[3(k-1)+2] (so chunk k-1's total has landed, page-locked output too);
//                 pageable: copies bounce block (k-1) & 1 out; pageable: host waits ev[3K+k-3], copies
//                 exception block (k-3) % 3 out; s_out: D2H of chunk k-1's exception words, sized by
//                 the total that came with it (none once that exceeds the caller's capacity), records
//                 ev[3K+k-1]
//   end           landed(K-1), the last two exception blocks' copy-out, the count; KW_E_NOSPACE when
//                 the words did not fit: the pass has run on and counted, and it stands
// (landed(k-2) for page-locked outputs was tried: the pass was no shorter, profiles/r09_bulk_packed.txt.)
struct PackedOut final : PlanesOut {
  static constexpr uint64_t kXRing = 4;  // slots of the device exception ring
  kw_packed* const pk;
  uint32_t *d_dict = nullptr, *d_tot = nullptr, *d_bsum = nullptr, *d_off = nullptr, *d_ibase = nullptr;
  volatile uint32_t* h_tot = nullptr;  // pinned; h_tot[k]: the exception words before chunk k
  size_t slot_words = 0, off_at = 0;   // a ring slot's words; the offsets' place in a bounce block
  std::vector<char> xissued;           // whether chunk k's exception read-back was issued
  bool nospace = false;
  explicit PackedOut(kw_packed* p) : PlanesOut(p->planes), pk(p) {}
  bool direct() const override { return page_locked(pk->planes) && page_locked(pk->exc_off) && page_locked(pk->exc); }
  uint32_t events_per_chunk() const override { return 4; }
  bool tolerates(int rc) const override { return rc == KW_E_NOSPACE; }
  void empty() override { pk->exc_off[0] = 0, pk->exc_count = 0; }
  int setup(const BulkCtx& c, uint64_t max_rows) override;
  int reduce(const BulkCtx& c, uint64_t k) override;
  int copies(const BulkCtx& c, uint64_t k) override;
  int landed(const BulkCtx& c, uint64_t k) override;
  int end(const BulkCtx& c) override;
  int copy_out_exc(const BulkCtx& c, uint64_t k);  // pageable: exception block k % 3 out, once chunk k's words are in it
};

// kw_validate_host_summary (summary.hpp): per-column counters and, where asked for, planes. The
// running u64 totals are zeroed on sc ahead of the first chunk.
//   reduce(k)     sc: the summary kernel over the chunk's rows (planes into the device plane array at
//                 the chunk's rows; none without planes), then the totals kernel, which adds the
//                 chunk's partial blocks into the running totals: ordered by sc, so chunk k+1's
//                 partial blocks overwrite chunk k's only after they were added
//   copies(k)     D2H of the chunk's planes into the caller's page-locked array or bounce block k & 1
//                 (no copy without planes)
//   landed(k-1)   (pageable planes) host waits ev[3(k-1)+2], copies bounce block (k-1) & 1 out
//   end           landed(K-1), then on s_out (which has waited for ev[3(K-1)+1], recorded behind the
//                 last totals kernel) the D2H of the totals into a pinned block, a host wait for
//                 s_out, the copy into the caller's col
// The verdict buffer keeps every chunk's words, so kw_batch_verdict_rows and kw_batch_verdicts work
// on the pass.
struct SummaryOut final : PlanesOut {
  kw_summary* const sm;
  uint64_t* d_tot = nullptr;   // the running totals [npol][KW_SUM_N]
  uint32_t* d_part = nullptr;  // the workgroups' partial blocks
  explicit SummaryOut(kw_summary* s) : PlanesOut(s->planes), sm(s) {}
  bool direct() const override { return !sm->planes || page_locked(sm->planes); }  // (no planes: only the totals go out)
  void empty() override { memset(sm->col, 0, summary_col_words(sm->npol) * 8); }
  int setup(const BulkCtx& c, uint64_t max_rows) override;
  int reduce(const BulkCtx& c, uint64_t k) override;
  int copies(const BulkCtx& c, uint64_t k) override { return copy_planes(c, k); }
  int landed(const BulkCtx& c, uint64_t k) override;
  int end(const BulkCtx& c) override;
};

}  // namespace kw
