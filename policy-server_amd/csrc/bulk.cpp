// bulk.cpp — bulk host -> host validation (kw_validate_host): the batch's columns are uploaded,
// evaluated and read back in row chunks whose stages overlap: the host workers build chunk k's tile
// descriptors and fill its pinned staging while the copy engines move chunk k-1 in and chunk k-2's
// verdicts out and the tile kernel evaluates in between (three streams ordered by events). Only the
// string columns the pass reads are uploaded. The plan's tile capacities come from a sample of the
// tile needs (every stride-th tile), and each chunk's descriptors are built just before its fill,
// so the first read-back starts after one small chunk rather than after a whole-batch head; a
// request that exceeds the capacities alone runs through the overflow kernels right after its
// chunk's tile launch. Passes with several launches, wide side data or NFA elements run unchunked
// (upload, pass, read-back) with the same result.
//
// The contract of a chunked pass: streams s_in (uploads), sc (the batch's stream: kernels) and
// s_out (read-back); chunk k of K owns events ev[3k] (uploaded), ev[3k+1] (evaluated) and ev[3k+2]
// (read back). Per chunk, in this order, on the calling thread:
//   stage_columns  host waits ev[3(k-depth)+2] (pinned output with a depth only)
//                  host waits ev[3(k-kRing)] (packed only: the ring slot's previous upload), fills
//                  s_in: H2D of each column range DMA'd in place; then either the packed slot's H2D
//                        and the scatter kernel, or one H2D per staged range
//   stage_descs    descriptors built on the host; more than the halves hold: host waits s_in and sc,
//                  regrows both halves; else host waits ev[3(k-2)] (the host half's previous upload)
//   launch         s_in: waits ev[3(k-2)+1] (the device half's previous kernel), descriptor H2D,
//                        records ev[3k]
//                  sc:   waits ev[3k], the tile kernel (none for a chunk without descriptors)
//   overflow       (chunks with overflow requests only) host waits sc, sc: zeroes the record count
//                  (first such chunk), buffers grown synchronously, blocking H2D of the list,
//                  sc: the overflow kernels
//   read_back      sc: records ev[3k+1]; s_out: waits ev[3k+1], D2H of the chunk's verdicts into the
//                  caller's pinned buffer or bounce block k & 1, records ev[3k+2]
//   copy_out(k-1)  (pageable output) host waits ev[3(k-1)+2], copies bounce block (k-1) & 1 out
// and after the last chunk copy_out(K-1), then the drain of s_in, sc, s_out — on every path,
// errors included — before any block, stream or event returns to its pool (Res).
//
// The packed output form (kw_validate_host_packed, packed.hpp) replaces read_back and copy_out:
// chunk k also owns ev[3K+k] (its exception words read back) and slot k % kXRing of the device
// exception ring. Per chunk, after launch / overflow:
//   pack           sc: waits ev[3K+k-kXRing] (the ring slot's previous read-back, where one was
//                  issued), the five pack kernels over the chunk's rows of the verdict buffer; the
//                  scan is seeded with the device-resident total chunk k-1's scan left
//   read_back      sc: records ev[3k+1]; s_out: waits ev[3k+1], D2H of the chunk's planes, offsets
//                  and its 4-byte running total (into the caller's pinned arrays or bounce block
//                  k & 1; the total into a pinned word per chunk), records ev[3k+2]
//   out(k-1)       host waits ev[3(k-1)+2] (so chunk k-1's total has landed); pageable: copies
//                  bounce block (k-1) & 1 out; pageable: host waits ev[3K+k-3], copies exception
//                  block (k-3) % 3 out; s_out: D2H of chunk k-1's exception words (none once the
//                  total exceeds the caller's capacity), records ev[3K+k-1]
// and after the last chunk out(K-1), the last two exception blocks' copy-out, then the same drain. A
// pass that runs unchunked packs its verdict buffer after the pass in row slabs by the same steps.
// (out(k-2) for page-locked outputs was tried: the pass was no shorter, profiles/r09_bulk_packed.txt.)
//
// The summary output form (kw_validate_host_summary, summary.hpp) replaces read_back and copy_out
// too; it needs no event beyond the three per chunk. The running u64 totals are zeroed on sc ahead of
// the first chunk. Per chunk, after launch / overflow:
//   summarize      sc: the summary kernel over the chunk's rows of the verdict buffer (planes into
//                  the device plane array at the chunk's rows; none without planes), then the totals
//                  kernel, which adds the chunk's partial blocks into the running totals: ordered by
//                  sc, so chunk k + 1's partial blocks overwrite chunk k's only after they were added
//   read_back      sc: records ev[3k+1]; s_out: waits ev[3k+1], D2H of the chunk's planes into the
//                  caller's page-locked array or bounce block k & 1 (no copy without planes), records
//                  ev[3k+2]
//   out(k-1)       (pageable planes) host waits ev[3(k-1)+2], copies bounce block (k-1) & 1 out
// and after the last chunk out(K-1), then on s_out (which has waited for ev[3(K-1)+1], recorded behind
// the last totals kernel) the D2H of the totals into a pinned block, a host wait for s_out, the copy
// into the caller's col, and the same drain. The verdict buffer keeps every chunk's words, so
// kw_batch_verdict_rows and kw_batch_verdicts work on the pass. A pass that runs unchunked is
// summarised after the pass in row slabs by the same steps.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <optional>

#include "bulkplan.hpp"
#include "knobs.hpp"
#include "packed.hpp"
#include "pass.hpp"
#include "plan.hpp"
#include "summary.hpp"
#include "upload.hpp"

namespace kw {
namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); }

// diagnostics (KW_BULK_DEBUG=1): host wall time of each stage in ms, printed at the end
struct BulkTimes {
  double layout = 0, plan = 0, prep = 0, desc = 0, fill = 0, enq = 0, out = 0, first = -1, wait = 0;
};

// staged columns: each chunk's ranges packed into one pinned slot, one H2D into the device slot,
// then the scatter kernel puts them in place (one copy per chunk, not one per column). kRing
// slots: packing chunk k waits for chunk k - kRing's upload. KW_BULK_PACK=0: a copy per column
// range (A/B knob, profiles/r05_bulk_copies.txt).
constexpr uint64_t kRing = 4;
// packed output: slots of the device exception ring (chunk k's pack waits for chunk k - kXRing's
// exception read-back, issued two chunks before it at the latest)
constexpr uint64_t kXRing = 4;

// What a chunked pass takes from the pools for the length of the call. The destructor drains the
// three streams; the leases are members, so they return to their pools after it on every path: a
// block returned while a copy into it is in flight would be handed to another thread's pass.
struct Res {
  hipStream_t sc;
  BlockLease dland, hpack;  // the landing ring on the device and the pack ring in pinned memory
  BlockLease hdesc;         // the pinned descriptor halves
  BlockLease bounce[2];     // pageable output: verdicts land here
  // packed output: the device arrays (dictionary, totals, scan sums, planes, offsets, item bases),
  // the exception ring, the pinned totals and dictionary, the pageable output's exception blocks
  // summary output: dfix holds the device planes, totals and partial blocks, hfix the pinned totals
  BlockLease dfix, dexc, hfix, xb[3];
  StreamLease s_out, s_in;
  EventLease ev;
  bool drained = false;
  explicit Res(hipStream_t c) : sc(c) {}
  ~Res() { drain(); }
  void drain() {
    if (drained) return;
    drained = true;
    if (s_in.s) (void)hipStreamSynchronize(s_in.s);
    (void)hipStreamSynchronize(sc);
    if (s_out.s) (void)hipStreamSynchronize(s_out.s);
  }
};

// The wide-record buffer grown to `cap` records (at least doubled), keeping the records earlier
// chunks wrote.
int grow_wide_rec(DeviceBatch& D, int device, size_t cap) {
  WideRec* old = D.wide_rec;
  const size_t old_cap = D.wide_rec_cap;
  D.wide_rec = nullptr;
  D.wide_rec_cap = 0;
  if (int rc = ensure(&D.wide_rec, &D.wide_rec_cap, std::max(cap, 2 * old_cap))) return rc;
  if (old) HIPCHK(hipMemcpy(D.wide_rec, old, old_cap * sizeof(WideRec), hipMemcpyDeviceToDevice));
  if (old) dev_pool().release(device, old, old_cap * sizeof(WideRec));
  return KW_OK;
}

struct BulkPass {
  // the call
  const kw_env* env;
  kw_batch* kb;
  const int32_t* policies;
  uint32_t npol;
  int origin, device;
  uint32_t* out;
  size_t count;
  uint32_t chunk_rows;
  const bool dbg = Knobs::on<KW_BULK_DEBUG>();
  const clk::time_point t_start = clk::now();
  BulkTimes t;
  // plan
  std::vector<Piece> pieces;
  std::vector<char> dma;  // per piece: page-locked in place, DMA'd from where it lies
  PassPlan pl;
  uint32_t need = 0;
  bool chunked = false, pack_knob = false;
  uint8_t* st = nullptr;  // the whole-batch staging image, where it is used
  hipStream_t sc = nullptr;
  EvalArgs A;
  // setup
  std::vector<uint64_t> tb;  // chunk k: tiles [tb[k], tb[k+1])
  uint64_t K = 0, depth = 0, dcap = 0;
  bool pinned = false, packed = false;
  size_t slot_bytes = 0;
  std::optional<Res> res;
  // per chunk: its descriptors and overflow list; overflow requests so far
  std::vector<TileDesc> cd;
  std::vector<uint32_t> co;
  uint64_t n_ovf = 0;
  // packed output (kw_validate_host_packed): pk set, `out` null. rb: chunk k covers rows
  // [rb[k], rb[k+1]); the device arrays of Res::dfix; the pinned totals (h_tot[k]: the exception
  // words before chunk k); the ring slot's words; whether chunk k's exception read-back was issued
  kw_packed* pk = nullptr;
  std::vector<uint64_t> rb;
  uint32_t G = 1;
  uint32_t *d_dict = nullptr, *d_tot = nullptr, *d_bsum = nullptr, *d_off = nullptr, *d_ibase = nullptr;
  uint64_t* d_planes = nullptr;
  volatile uint32_t* h_tot = nullptr;
  size_t slot_words = 0, off_at = 0;  // off_at: the offsets' place in a bounce block
  std::vector<char> xissued;
  bool nospace = false;
  // summary output (kw_validate_host_summary): sm set, `out` null; rb, G and d_planes as above; the
  // running totals [npol][KW_SUM_N] and the workgroups' partial blocks (Res::dfix)
  kw_summary* sm = nullptr;
  uint64_t* d_stot = nullptr;
  uint32_t* d_spart = nullptr;

  BulkPass(const kw_env* e, kw_batch* b, const int32_t* p, uint32_t np, int o, int dev, uint32_t* w, size_t c, uint32_t cr)
      : env(e), kb(b), policies(p), npol(np), origin(o), device(dev), out(w), count(c), chunk_rows(cr) {}

  uint64_t row_of(uint64_t tile) const { return std::min<uint64_t>(kb->b.n, tile * pl.geom.rows); }

  // A non-empty byte range [lo, hi) of a piece the pass reads.
  struct Range {
    size_t piece, lo, hi;
  };
  std::vector<Range> ranges(uint64_t k) const {
    std::vector<Range> v;
    for (size_t i = 0; i < pieces.size(); ++i) {
      const Piece& p = pieces[i];
      if (p.m >= 0 && !((need >> p.m) & 1u)) continue;
      size_t lo, hi;
      piece_range(kb->b, p, row_of(tb[k]), row_of(tb[k + 1]), k + 1 == K, &lo, &hi);
      if (hi > lo) v.push_back({i, lo, hi});
    }
    return v;
  }

  // Layout, the plan from sampled tile needs, the columns to DMA in place, chunked or not.
  int plan() {
    if (int rc = layout_batch(kb, device, nullptr, &pieces, /*may_split=*/false, /*staging=*/false)) return rc;
    t.layout = since(t_start);
    DeviceBatch& D = *kb->dev;
    const Batch& B = kb->b;
    D.loaded = ~0u;  // (planned as if resident; set to the pass's columns below)
    // tile capacities from about 2048 sampled tiles (KW_BULK_SAMPLE=0: every tile, A/B knob)
    const bool sample = Knobs::on<KW_BULK_SAMPLE>();
    D.needs_stride = sample ? (uint32_t)std::max<uint64_t>(1, B.n / ((uint64_t)kSlotRows * 2048)) : 1u;
    const int prc = validate_common(env, kb, policies, npol, nullptr, origin, &pl);
    D.needs_stride = 1;
    if (prc) {
      D.loaded = 0;
      return prc;
    }
    need = pl.geom.need;
    t.plan = since(t_start) - t.layout;
    // columns page-locked in place (kw_batch_pin_host) go to the device by DMA from where they lie;
    // the others through the pinned staging, filled by the host workers
    dma.assign(pieces.size(), 0);
    if (!kb->host_pinned.empty())
      for (size_t i = 0; i < pieces.size(); ++i) dma[i] = pieces[i].bytes && page_locked(pieces[i].src);
    sc = D.stream;
    // (NFA elements: their pre-pass reads whole columns, so such passes are not chunked)
    chunked = pl.tiles.size() == 1 && pl.wide.groups.empty() && pl.nwide == 0 && !pl.rows_mode &&
              !(pl.geom.debug & 512u) && !(pl.geom.feat & kFeatNfa) && B.n > 0;
    // the staging image of the whole batch only where it is used: the unchunked path and per-range
    // copies (packed chunks go through their own ring; pinning C5's 3.6 GB image cost 360 ms a call)
    pack_knob = Knobs::on<KW_BULK_PACK>();
    if ((!chunked || !pack_knob) && !D.staging) {
      HIPCHK(host_pool().alloc(device, D.cols_bytes, &D.staging));
      D.staging_bytes = D.cols_bytes;
    }
    st = (uint8_t*)D.staging;
    return KW_OK;
  }

  // One upload, the full pass.
  int run_whole() {
    DeviceBatch& D = *kb->dev;
    std::vector<CopySeg> segs;
    for (size_t i = 0; i < pieces.size(); ++i)
      if (pieces[i].bytes && !dma[i]) segs.push_back({st + pieces[i].at, pieces[i].src, pieces[i].bytes});
    parallel_copy_segs(segs);
    for (const CopySeg& c : segs)
      HIPCHK(hipMemcpyAsync(D.cols + ((uint8_t*)c.dst - st), c.dst, c.bytes, hipMemcpyHostToDevice, sc));
    for (size_t i = 0; i < pieces.size(); ++i)
      if (pieces[i].bytes && dma[i])
        HIPCHK(hipMemcpyAsync(D.cols + pieces[i].at, pieces[i].src, pieces[i].bytes, hipMemcpyHostToDevice, sc));
    return run_validate(env, kb, pl, origin, false, sc);
  }

  // One upload, the full pass, one read-back.
  int run_unchunked() {
    if (int rc = run_whole()) return rc;
    return read_verdicts(kb, out, count);
  }

  // The plan onto the device; descriptors follow per chunk.
  int prepare() {
    DeviceBatch& D = *kb->dev;
    D.last_big_stride = 0;  // (no wide groups in a chunked pass: stale cause bitsets must not be read)
    D.last_big_ref.clear();
    if (int rc = prepare_pass(kb, pl, sc, &A, /*descs=*/false)) {
      D.loaded = 0;
      return rc;
    }
    t.prep = since(t_start) - t.layout - t.plan;
    D.loaded = need;
    return KW_OK;
  }

  // Descriptors: two halves of `dcap` on the device and in pinned host memory (chunk k uses half
  // k & 1; half reuse waits for chunk k-2's kernel on the device and its upload on the host).
  int alloc_descs() {
    DeviceBatch& D = *kb->dev;
    HIPCHK(res->hdesc.alloc(host_pool(), device, (size_t)(2 * dcap) * sizeof(TileDesc)));
    return ensure(&D.desc, &D.desc_cap, (size_t)(2 * dcap));
  }

  // The chunk schedule and what the chunks share: bounce blocks, descriptor halves, the packed
  // ring, streams and events. From here on a failure leaves the batch's columns partly uploaded
  // (finish clears D.loaded).
  int setup() {
    const TileArgs& G = pl.geom;
    const uint64_t ntiles = (kb->b.n + G.rows - 1) / G.rows;
    const uint64_t def_chunk = (uint64_t)Knobs::num<KW_BULK_CHUNK>();  // A/B knob (profiles/r04_bulk_sweep.txt)
    const uint64_t per = chunk_rows ? chunk_rows : def_chunk;
    const bool ramp = Knobs::on<KW_BULK_RAMP>();  // A/B knob
    const uint64_t tper = chunk_tiles(ntiles, G.rows, per);
    tb = chunk_bounds(ntiles, G.rows, per, ramp);
    K = tb.size() - 1;
    const bool direct = Knobs::on<KW_BULK_DIRECT>();  // A/B knob
    pinned = direct && (pk   ? packed_pinned()
                        : sm ? summary_pinned()
                             : page_locked(out));
    const int depth_knob = Knobs::num<KW_BULK_DEPTH>();  // A/B knob, 0 = unbounded
    depth = bulk_depth(depth_knob, std::count(dma.begin(), dma.end(), 1) > 0);
    // (the largest chunk: `per` grows past ~240 chunks)
    uint64_t max_rows = 0;
    for (uint64_t k = 0; k < K; ++k) max_rows = std::max(max_rows, row_of(tb[k + 1]) - row_of(tb[k]));
    dcap = tper + tper / 4 + 64;
    res.emplace(sc);
    if (!pinned && !pk && !sm)
      for (BlockLease& b : res->bounce) HIPCHK(b.alloc(host_pool(), device, (size_t)max_rows * npol * 4));
    if (pk) {
      for (uint64_t k = 0; k <= K; ++k) rb.push_back(row_of(tb[k]));
      if (int rc = setup_packed(max_rows)) return rc;
    }
    if (sm) {
      for (uint64_t k = 0; k <= K; ++k) rb.push_back(row_of(tb[k]));
      if (int rc = setup_summary(max_rows)) return rc;
    }
    if (int rc = alloc_descs()) return rc;
    // (the scatter kernel's argument holds kMaxScatterSegs ranges: a layout with more staged pieces
    // than that — none today, 6 row pieces + 2 per string column — copies each range on its own)
    packed = pack_knob && std::count(dma.begin(), dma.end(), 0) > 0 &&
             (size_t)std::count(dma.begin(), dma.end(), 0) <= kMaxScatterSegs;
    if (packed) {
      for (uint64_t k = 0; k < K; ++k) {
        std::vector<PackRange> pr;
        for (const Range& r : ranges(k))
          if (!dma[r.piece]) pr.push_back({pieces[r.piece].at + r.lo, r.hi - r.lo});
        slot_bytes = std::max<size_t>(slot_bytes, slot_estimate(pr));
      }
      HIPCHK(res->hpack.alloc(host_pool(), device, kRing * slot_bytes));
      HIPCHK(res->dland.alloc(dev_pool(), device, kRing * slot_bytes));
    }
    HIPCHK(res->s_in.get(device));
    HIPCHK(res->s_out.get(device));
    HIPCHK(res->ev.get(device, (pk ? 4 : 3) * K));
    return KW_OK;
  }

  // ---- packed output ----

  // Direct DMA only when all three output arrays are page-locked.
  bool packed_pinned() const {
    return page_locked(pk->planes) && page_locked(pk->exc_off) && page_locked(pk->exc);
  }

  // The packed form's blocks for chunks of at most max_rows rows (rb, K and `pinned` are set), the
  // dictionary onto the device and the running total zeroed, both on sc ahead of the first pack.
  int setup_packed(uint64_t max_rows) {
    const uint64_t rows = kb->b.n, items = packed_items(rows, npol);
    G = packed_groups(npol);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_dict = up((size_t)npol * 12), b_tot = up((K + 1) * 4);
    const size_t b_bsum = up(((size_t)max_rows * G / kScanBlock + 1) * 4), b_planes = up((size_t)items * 16);
    const size_t b_off = up((size_t)(rows + 1) * 4), b_ibase = up((size_t)items * 4);
    HIPCHK(res->dfix.alloc(dev_pool(), device, b_dict + b_tot + b_bsum + b_planes + b_off + b_ibase));
    uint8_t* d = (uint8_t*)res->dfix.p;
    d_planes = (uint64_t*)d, d += b_planes;
    d_dict = (uint32_t*)d, d += b_dict;
    d_tot = (uint32_t*)d, d += b_tot;
    d_bsum = (uint32_t*)d, d += b_bsum;
    d_off = (uint32_t*)d, d += b_off;
    d_ibase = (uint32_t*)d;
    slot_words = (size_t)max_rows * npol;
    HIPCHK(res->dexc.alloc(dev_pool(), device, kXRing * slot_words * 4));
    HIPCHK(res->hfix.alloc(host_pool(), device, b_tot + b_dict));
    h_tot = (volatile uint32_t*)res->hfix.p;
    for (uint64_t k = 0; k <= K; ++k) h_tot[k] = 0;
    uint32_t* h_dict = (uint32_t*)((uint8_t*)res->hfix.p + b_tot);
    memcpy(h_dict, pk->dict, (size_t)npol * 12);
    off_at = up((size_t)max_rows * G * 16);
    if (!pinned) {
      for (BlockLease& b : res->bounce) HIPCHK(b.alloc(host_pool(), device, off_at + (size_t)(max_rows + 1) * 4));
      for (BlockLease& b : res->xb) HIPCHK(b.alloc(host_pool(), device, std::max<size_t>(slot_words, 1) * 4));
    }
    xissued.assign(K, 0);
    HIPCHK(hipMemcpyAsync(d_dict, h_dict, (size_t)npol * 12, hipMemcpyHostToDevice, sc));
    HIPCHK(hipMemsetAsync(d_tot, 0, 4, sc));
    return KW_OK;
  }

  hipEvent_t evx(uint64_t k) const { return res->ev[3 * K + k]; }

  // The chunk's words packed on the device behind its kernels.
  int pack(uint64_t k) {
    DeviceBatch& D = *kb->dev;
    const uint64_t r0 = rb[k], r1 = rb[k + 1];
    if (k >= kXRing && xissued[k - kXRing]) HIPCHK(hipStreamWaitEvent(sc, evx(k - kXRing), 0));  // ring slot free
    PackArgs a;
    a.words = D.verdicts + r0 * npol;
    a.dict = d_dict;
    a.planes = d_planes + 2 * r0 * G;
    a.ibase = d_ibase + r0 * G;
    a.exc_off = d_off + r0;
    a.bsum = d_bsum;
    a.tot = d_tot + k;
    a.exc = (uint32_t*)res->dexc.p + (k % kXRing) * slot_words;
    a.exc_cap = (uint32_t)std::min<uint64_t>((r1 - r0) * npol, slot_words);
    a.npol = npol;
    a.G = G;
    a.nitems = (uint32_t)((r1 - r0) * G);
    if (r1 == r0) {  // (no rows: the total passes through)
      HIPCHK(hipMemcpyAsync(d_tot + k + 1, d_tot + k, 4, hipMemcpyDeviceToDevice, sc));
      return KW_OK;
    }
    HIPCHK(launch_pack(a, sc));
    return KW_OK;
  }

  // The chunk's planes, offsets and running total to the host behind its pack kernels.
  int read_back_packed(uint64_t k) {
    const EventLease& ev = res->ev;
    hipStream_t s_out = res->s_out.s;
    const uint64_t r0 = rb[k], r1 = rb[k + 1];
    const uint64_t noff = r1 - r0 + (k + 1 == K ? 1 : 0);  // (the last chunk brings the final total)
    HIPCHK(hipEventRecord(ev[3 * k + 1], sc));
    HIPCHK(hipStreamWaitEvent(s_out, ev[3 * k + 1], 0));
    uint8_t* bb = pinned ? nullptr : (uint8_t*)res->bounce[k & 1].p;
    if (r1 > r0)
      HIPCHK(hipMemcpyAsync(pinned ? (void*)(pk->planes + 2 * r0 * G) : (void*)bb, d_planes + 2 * r0 * G,
                            (size_t)(r1 - r0) * G * 16, hipMemcpyDeviceToHost, s_out));
    if (noff)
      HIPCHK(hipMemcpyAsync(pinned ? (void*)(pk->exc_off + r0) : (void*)(bb + off_at), d_off + r0, (size_t)noff * 4,
                            hipMemcpyDeviceToHost, s_out));
    HIPCHK(hipMemcpyAsync((void*)(h_tot + k + 1), d_tot + k + 1, 4, hipMemcpyDeviceToHost, s_out));
    HIPCHK(hipEventRecord(ev[3 * k + 2], s_out));
    return KW_OK;
  }

  // Pageable output: exception block k % 3 to the caller's array, once chunk k's words are in it.
  int copy_out_exc(uint64_t k) {
    if (pinned || !xissued[k]) return KW_OK;
    HIPCHK(hipEventSynchronize(evx(k)));
    parallel_copy_segs({{pk->exc + h_tot[k], res->xb[k % 3].p, (size_t)(h_tot[k + 1] - h_tot[k]) * 4}});
    return KW_OK;
  }

  // The chunk's fixed-size parts have landed: out of their bounce block (pageable), then its
  // exception words' read-back, sized by the total that came with them.
  int out_packed(uint64_t k) {
    const auto t0 = clk::now();
    HIPCHK(hipEventSynchronize(res->ev[3 * k + 2]));
    const uint64_t r0 = rb[k], r1 = rb[k + 1];
    if (!pinned) {
      const uint8_t* bb = (const uint8_t*)res->bounce[k & 1].p;
      const uint64_t noff = r1 - r0 + (k + 1 == K ? 1 : 0);
      parallel_copy_segs({{pk->planes + 2 * r0 * G, bb, (size_t)(r1 - r0) * G * 16}, {pk->exc_off + r0, bb + off_at, (size_t)noff * 4}});
      if (k >= 2)  // (two steps behind its read-back: the host does not wait for a copy just queued)
        if (int rc = copy_out_exc(k - 2)) return rc;
    }
    const uint32_t t_lo = h_tot[k], t_hi = h_tot[k + 1];
    if (t_hi > pk->exc_cap) nospace = true;  // (the pass goes on and counts)
    if (!nospace && t_hi > t_lo) {
      const uint32_t* src = (const uint32_t*)res->dexc.p + (k % kXRing) * slot_words;
      HIPCHK(hipMemcpyAsync(pinned ? (void*)(pk->exc + t_lo) : res->xb[k % 3].p, src, (size_t)(t_hi - t_lo) * 4,
                            hipMemcpyDeviceToHost, res->s_out.s));
      HIPCHK(hipEventRecord(evx(k), res->s_out.s));
      xissued[k] = 1;
    }
    t.out += since(t0);
    return KW_OK;
  }

  // After the last chunk: its exception words out; the count, and whether they fitted.
  int end_packed() {
    if (K) {
      if (int rc = out_packed(K - 1)) return rc;
      if (K >= 2)
        if (int rc = copy_out_exc(K - 2)) return rc;
      if (int rc = copy_out_exc(K - 1)) return rc;
      if (xissued[K - 1]) HIPCHK(hipEventSynchronize(evx(K - 1)));
    }
    pk->exc_count = K ? h_tot[K] : 0;
    return nospace ? KW_E_NOSPACE : KW_OK;
  }

  // A pass that ran unchunked (run_unchunked's upload and pass): its verdict buffer packed in row
  // slabs through the chunked form's steps.
  int run_unchunked_packed() {
    if (int rc = run_whole()) return rc;
    const uint64_t rows = kb->b.n, per = chunk_rows ? chunk_rows : (uint64_t)Knobs::num<KW_BULK_CHUNK>();
    const uint64_t slab = std::max<uint64_t>({1, per, (rows + 239) / 240});
    for (uint64_t r = 0; r < rows; r += slab) rb.push_back(r);
    rb.push_back(rows);
    K = rb.size() - 1;
    if (K == 0) {
      pk->exc_off[0] = 0;
      pk->exc_count = 0;
      return load_side_data(kb, sc);
    }
    pinned = Knobs::on<KW_BULK_DIRECT>() && packed_pinned();
    res.emplace(sc);
    int rc = setup_packed(std::min(slab, rows));
    if (rc == KW_OK) rc = res->s_out.get(device) == hipSuccess && res->ev.get(device, 4 * K) == hipSuccess ? KW_OK : KW_E_DEVICE;
    for (uint64_t k = 0; k < K && rc == KW_OK; ++k) {
      rc = pack(k);
      if (rc == KW_OK) rc = read_back_packed(k);
      if (rc == KW_OK && k >= 1) rc = out_packed(k - 1);
    }
    if (rc == KW_OK) rc = end_packed();
    res->drain();
    res.reset();
    if (rc != KW_OK && rc != KW_E_NOSPACE) return rc;
    const int src = load_side_data(kb, sc);
    return src ? src : rc;
  }

  // ---- summary output ----

  // Direct DMA when the planes are page-locked (without planes nothing but the totals goes out).
  bool summary_pinned() const { return !sm->planes || page_locked(sm->planes); }

  // The summary form's blocks for chunks of at most max_rows rows (rb, K and `pinned` are set) and
  // the running totals zeroed on sc ahead of the first summary kernel.
  int setup_summary(uint64_t max_rows) {
    const uint64_t rows = kb->b.n;
    G = packed_groups(npol);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_tot = up(summary_col_words(npol) * 8), b_part = up(summary_part_bytes(max_rows, npol));
    const size_t b_planes = sm->planes ? up((size_t)rows * G * 16) : 0;
    HIPCHK(res->dfix.alloc(dev_pool(), device, b_planes + b_tot + b_part));
    uint8_t* d = (uint8_t*)res->dfix.p;
    d_planes = (uint64_t*)d, d += b_planes;
    d_stot = (uint64_t*)d, d += b_tot;
    d_spart = (uint32_t*)d;
    HIPCHK(res->hfix.alloc(host_pool(), device, b_tot));
    if (!pinned && sm->planes)
      for (BlockLease& b : res->bounce) HIPCHK(b.alloc(host_pool(), device, std::max<size_t>((size_t)max_rows * G * 16, 16)));
    HIPCHK(hipMemsetAsync(d_stot, 0, summary_col_words(npol) * 8, sc));
    return KW_OK;
  }

  // The chunk's words reduced on the device behind its kernels, into the running totals.
  int summarize(uint64_t k) {
    DeviceBatch& D = *kb->dev;
    const uint64_t r0 = rb[k], r1 = rb[k + 1];
    SumArgs a;
    a.words = D.verdicts + r0 * npol;
    a.planes = sm->planes ? d_planes + 2 * r0 * G : nullptr;
    a.part = d_spart;
    a.tot = d_stot;
    a.rows = r1 - r0;
    a.npol = npol;
    HIPCHK(launch_summary(a, sc));
    return KW_OK;
  }

  // The chunk's planes to the host behind its summary kernels.
  int read_back_summary(uint64_t k) {
    const EventLease& ev = res->ev;
    hipStream_t s_out = res->s_out.s;
    const uint64_t r0 = rb[k], r1 = rb[k + 1];
    HIPCHK(hipEventRecord(ev[3 * k + 1], sc));
    HIPCHK(hipStreamWaitEvent(s_out, ev[3 * k + 1], 0));
    if (sm->planes && r1 > r0)
      HIPCHK(hipMemcpyAsync(pinned ? (void*)(sm->planes + 2 * r0 * G) : res->bounce[k & 1].p, d_planes + 2 * r0 * G,
                            (size_t)(r1 - r0) * G * 16, hipMemcpyDeviceToHost, s_out));
    HIPCHK(hipEventRecord(ev[3 * k + 2], s_out));
    return KW_OK;
  }

  // Pageable planes: the chunk's from its bounce block to the caller's array.
  int out_summary(uint64_t k) {
    if (pinned || !sm->planes) return KW_OK;  // (KW_BULK_DIRECT=0 clears `pinned` for a counters-only pass too)
    const auto t0 = clk::now();
    HIPCHK(hipEventSynchronize(res->ev[3 * k + 2]));
    const uint64_t r0 = rb[k], r1 = rb[k + 1];
    parallel_copy_segs({{sm->planes + 2 * r0 * G, res->bounce[k & 1].p, (size_t)(r1 - r0) * G * 16}});
    t.out += since(t0);
    return KW_OK;
  }

  // After the last chunk: its planes out, then the totals, read back once.
  int end_summary() {
    if (K)
      if (int rc = out_summary(K - 1)) return rc;
    const size_t b_tot = summary_col_words(npol) * 8;
    hipStream_t s_out = res->s_out.s;  // (has waited for the last chunk's ev[3k+1], behind its totals kernel)
    HIPCHK(hipMemcpyAsync(res->hfix.p, d_stot, b_tot, hipMemcpyDeviceToHost, s_out));
    HIPCHK(hipStreamSynchronize(s_out));
    memcpy(sm->col, res->hfix.p, b_tot);
    return KW_OK;
  }

  // A pass that ran unchunked: its verdict buffer summarised in row slabs through the chunked form's
  // steps.
  int run_unchunked_summary() {
    if (int rc = run_whole()) return rc;
    const uint64_t rows = kb->b.n, per = chunk_rows ? chunk_rows : (uint64_t)Knobs::num<KW_BULK_CHUNK>();
    const uint64_t slab = std::max<uint64_t>({1, per, (rows + 239) / 240});
    for (uint64_t r = 0; r < rows; r += slab) rb.push_back(r);
    rb.push_back(rows);
    K = rb.size() - 1;
    if (K == 0) {
      memset(sm->col, 0, summary_col_words(npol) * 8);
      return load_side_data(kb, sc);
    }
    pinned = Knobs::on<KW_BULK_DIRECT>() && summary_pinned();
    res.emplace(sc);
    int rc = setup_summary(std::min(slab, rows));
    if (rc == KW_OK) rc = res->s_out.get(device) == hipSuccess && res->ev.get(device, 3 * K) == hipSuccess ? KW_OK : KW_E_DEVICE;
    for (uint64_t k = 0; k < K && rc == KW_OK; ++k) {
      rc = summarize(k);
      if (rc == KW_OK) rc = read_back_summary(k);
      if (rc == KW_OK && k >= 1) rc = out_summary(k - 1);
    }
    if (rc == KW_OK) rc = end_summary();
    res->drain();
    res.reset();
    if (rc != KW_OK) return rc;
    return load_side_data(kb, sc);
  }

  // The chunk's columns: their H2D starts at once, and the descriptor build after it then reads
  // offsets the fill has just brought into the host caches.
  int stage_columns(uint64_t k) {
    DeviceBatch& D = *kb->dev;
    const EventLease& ev = res->ev;
    hipStream_t s_in = res->s_in.s;
    // pinned output: at most `depth` chunks in flight past the read-back
    if (pinned && depth && k >= depth) HIPCHK(hipEventSynchronize(ev[3 * (k - depth) + 2]));
    std::vector<CopySeg> segs, dsegs;  // (staged, direct)
    std::vector<PackRange> pr;         // the staged ranges in the device image
    for (const Range& r : ranges(k)) {
      const Piece& p = pieces[r.piece];
      const uint8_t* src = (const uint8_t*)p.src + r.lo;
      if (dma[r.piece]) {
        dsegs.push_back({D.cols + p.at + r.lo, src, r.hi - r.lo});
      } else {
        segs.push_back({packed ? nullptr : st + p.at + r.lo, src, r.hi - r.lo});
        pr.push_back({p.at + r.lo, r.hi - r.lo});
      }
    }
    const size_t slot = (size_t)(k % kRing) * slot_bytes;
    uint8_t *hslot = (uint8_t*)res->hpack.p + slot, *dslot = (uint8_t*)res->dland.p + slot;
    ScatterArgs sa;
    sa.dst = D.cols;
    sa.src = dslot;
    sa.nseg = 0;
    size_t pk = 0;  // packed bytes of the chunk (each range at its device offset's residue mod 16)
    if (packed) {
      std::vector<uint64_t> at;
      pk = pack_ranges(pr, &at);
      for (size_t i = 0; i < pr.size(); ++i) {
        segs[i].dst = hslot + at[i];
        sa.seg[sa.nseg++] = {pr[i].dev_off, at[i], pr[i].len};
      }
      if (k >= kRing) HIPCHK(hipEventSynchronize(ev[3 * (k - kRing)]));  // its slot's upload is done
    }
    const auto t0 = clk::now();
    parallel_copy_segs(segs);
    t.fill += since(t0);
    const auto t1 = clk::now();
    for (const CopySeg& c : dsegs) HIPCHK(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyHostToDevice, s_in));
    if (packed) {
      if (pk) {
        HIPCHK(hipMemcpyAsync(dslot, hslot, pk, hipMemcpyHostToDevice, s_in));
        HIPCHK(launch_scatter(sa, s_in));
      }
    } else {
      for (const CopySeg& c : segs)
        HIPCHK(hipMemcpyAsync(D.cols + ((uint8_t*)c.dst - st), c.dst, c.bytes, hipMemcpyHostToDevice, s_in));
    }
    t.enq += since(t1);
    return KW_OK;
  }

  // The chunk's descriptors and overflow list, the descriptors into their pinned half.
  int stage_descs(uint64_t k) {
    const auto td = clk::now();
    cd.clear();
    co.assign(1, 0u);
    if (int rc = build_descs(kb->b, pl.geom, 0, kb->b.n, tb[k], tb[k + 1], 128, 0, &cd, &co)) return rc;  // (fixed cut: pass.cpp)
    co[0] = (uint32_t)(co.size() - 1);
    if (cd.size() > dcap) {  // more split tiles than the halves hold: wait for every launch, regrow
      HIPCHK(hipStreamSynchronize(res->s_in.s));
      HIPCHK(hipStreamSynchronize(sc));
      dcap = cd.size() + cd.size() / 4 + 64;
      if (int rc = alloc_descs()) return rc;
    } else if (k >= 2) {  // host half free: its upload is done
      HIPCHK(hipEventSynchronize(res->ev[3 * (k - 2)]));
    }
    if (!cd.empty()) memcpy((TileDesc*)res->hdesc.p + (k & 1) * dcap, cd.data(), cd.size() * sizeof(TileDesc));
    t.desc += since(td);
    return KW_OK;
  }

  // The descriptors to the device behind the chunk's columns, the tile kernel behind both.
  int launch(uint64_t k) {
    DeviceBatch& D = *kb->dev;
    const EventLease& ev = res->ev;
    hipStream_t s_in = res->s_in.s;
    const TileDesc* hd = (const TileDesc*)res->hdesc.p + (k & 1) * dcap;
    TileDesc* dd = D.desc + (k & 1) * dcap;
    if (k >= 2) HIPCHK(hipStreamWaitEvent(s_in, ev[3 * (k - 2) + 1], 0));  // device half free
    if (!cd.empty()) HIPCHK(hipMemcpyAsync(dd, hd, cd.size() * sizeof(TileDesc), hipMemcpyHostToDevice, s_in));
    HIPCHK(hipEventRecord(ev[3 * k], s_in));
    HIPCHK(hipStreamWaitEvent(sc, ev[3 * k], 0));
    EvalArgs Ak = A;
    Ak.ndesc = cd.size();
    // (strided, or the counters from the third tile on: a chunk's few rounds take no counter-drawn tail)
    if (!sched_dynamic(cd.size(), pl.grid, pl.geom.lds_tables != 0)) Ak.sched = nullptr;
    if (!cd.empty()) HIPCHK(launch_evaluate_tiles(Ak, pl.tiles[0], D.d_tiles, dd, pl.grid, sc));
    return KW_OK;
  }

  // Overflow requests (alone beyond the tile capacities): rare, so a synchronous set-up of their
  // list, classes and side data, then the overflow kernels on the chunk's requests.
  int overflow() {
    DeviceBatch& D = *kb->dev;
    HIPCHK(hipStreamSynchronize(sc));
    if (n_ovf == 0) HIPCHK(hipMemsetAsync(D.wide_count, 0, sizeof(uint32_t), sc));  // (first overflow chunk)
    D.wide_valid = true;
    n_ovf += co[0];
    if (int rc = ensure(&D.overflow, &D.overflow_cap, co.size())) return rc;
    if (int rc = ensure_overflow_classes(kb->b, &D, pl.geom, &A)) return rc;
    const size_t cap = (size_t)n_ovf * pl.wide_cap_per_row;
    if (cap > D.wide_rec_cap || !D.wide_rec)
      if (int rc = grow_wide_rec(D, device, cap)) return rc;
    A.wide_rec = D.wide_rec;
    A.wide_cap = (uint32_t)std::min<size_t>(D.wide_rec_cap, 0xffffffffu);
    HIPCHK(hipMemcpy(D.overflow, co.data(), co.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(launch_overflow(A, D.d_tiles, D.overflow, co[0], sc));
    return KW_OK;
  }

  // The chunk's verdicts to the host behind its kernels.
  int read_back(uint64_t k) {
    DeviceBatch& D = *kb->dev;
    const EventLease& ev = res->ev;
    hipStream_t s_out = res->s_out.s;
    const uint64_t r0 = row_of(tb[k]), r1 = row_of(tb[k + 1]);
    HIPCHK(hipEventRecord(ev[3 * k + 1], sc));
    HIPCHK(hipStreamWaitEvent(s_out, ev[3 * k + 1], 0));
    uint32_t* dst = pinned ? out + r0 * npol : (uint32_t*)res->bounce[k & 1].p;
    HIPCHK(hipMemcpyAsync(dst, D.verdicts + r0 * npol, (size_t)(r1 - r0) * npol * 4, hipMemcpyDeviceToHost, s_out));
    HIPCHK(hipEventRecord(ev[3 * k + 2], s_out));
    return KW_OK;
  }

  // Pageable output: the chunk's verdicts from its bounce block to the caller's buffer.
  int copy_out(uint64_t k) {
    const auto t0 = clk::now();
    if (pinned) return KW_OK;
    HIPCHK(hipEventSynchronize(res->ev[3 * k + 2]));
    const uint64_t r0 = row_of(tb[k]), r1 = row_of(tb[k + 1]);
    parallel_copy_segs({{out + r0 * npol, res->bounce[k & 1].p, (size_t)(r1 - r0) * npol * 4}});
    t.out += since(t0);
    return KW_OK;
  }

  int chunk(uint64_t k) {
    if (int rc = stage_columns(k)) return rc;
    if (int rc = stage_descs(k)) return rc;
    const auto t2 = clk::now();
    if (int rc = launch(k)) return rc;
    if (co[0])
      if (int rc = overflow()) return rc;
    if (pk) {
      if (int rc = pack(k)) return rc;
      if (int rc = read_back_packed(k)) return rc;
    } else if (sm) {
      if (int rc = summarize(k)) return rc;
      if (int rc = read_back_summary(k)) return rc;
    } else if (int rc = read_back(k)) {
      return rc;
    }
    t.enq += since(t2);
    if (k == 0) t.first = since(t_start);
    if (pk) return k >= 1 ? out_packed(k - 1) : KW_OK;
    if (sm) return k >= 1 ? out_summary(k - 1) : KW_OK;
    return k >= 1 ? copy_out(k - 1) : KW_OK;  // (bounce[k & 1] was last read by chunk k - 2's copy-out)
  }

  // The drain, the per-call resources back to their pools, the side data; rc: the chunks' result.
  int finish(int rc) {
    DeviceBatch& D = *kb->dev;
    const auto t_w = clk::now();
    res->drain();
    t.wait = since(t_w);
    const auto t_td = clk::now();
    res.reset();
    D.last_wide_cap = A.wide_cap;
    D.cur = sc;
    if (rc != KW_OK && !(pk && rc == KW_E_NOSPACE)) {
      D.loaded = 0;
      return rc;
    }
    if (int src = load_side_data(kb, sc)) rc = src;  // overflow requests' wide arguments (kw_batch_wide_arg)
    if (dbg && pk)
      fprintf(stderr, "[kw bulk] packed: %llu exception words of %llu (capacity %llu), %.1f B per row read back\n",
              (unsigned long long)pk->exc_count, (unsigned long long)count, (unsigned long long)pk->exc_cap,
              kb->b.n ? ((double)pk->exc_count * 4 + (double)kb->b.n * (G * 16 + 4)) / (double)kb->b.n : 0.0);
    if (dbg)
      fprintf(stderr,
              "[kw bulk] rows %llu chunks %llu pinned %d direct-columns %d overflow %llu: layout %.2f plan %.2f prepare %.2f "
              "descs %.2f fill %.2f enqueue %.2f copy-out %.2f first chunk queued at %.2f, final wait %.2f, teardown %.2f, "
              "total %.2f ms\n",
              (unsigned long long)kb->b.n, (unsigned long long)K, pinned ? 1 : 0, (int)std::count(dma.begin(), dma.end(), 1),
              (unsigned long long)n_ovf, t.layout, t.plan, t.prep, t.desc, t.fill, t.enq, t.out, t.first, t.wait, since(t_td),
              since(t_start));
    return rc;
  }
};

}  // namespace

int validate_host(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, int device,
                  uint32_t* out, size_t count, uint32_t chunk_rows) {
  if (!env || !kb || !out || !policies || npol == 0) return KW_E_ARG;
  if (env->e.device < 0 || !env->e.d_blob) return KW_E_DEVICE;
  if (device != env->e.device || count != kb->b.n * (uint64_t)npol) return KW_E_ARG;
  BulkPass P(env, kb, policies, npol, origin, device, out, count, chunk_rows);
  if (int rc = P.plan()) return rc;
  if (!P.chunked) return P.run_unchunked();
  if (int rc = P.prepare()) return rc;
  int rc = P.setup();
  for (uint64_t k = 0; k < P.K && rc == KW_OK; ++k) rc = P.chunk(k);
  if (rc == KW_OK) rc = P.copy_out(P.K - 1);
  return P.finish(rc);
}

int validate_host_packed(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, int device,
                         kw_packed* out, uint32_t chunk_rows) {
  if (!env || !kb || !out || !policies || npol == 0) return KW_E_ARG;
  if (env->e.device < 0 || !env->e.d_blob) return KW_E_DEVICE;
  if (device != env->e.device || out->rows != kb->b.n || out->npol != npol || !packed_fits(out->rows, npol)) return KW_E_ARG;
  if (!out->dict || !out->exc_off || (out->rows && !out->planes) || (out->exc_cap && !out->exc)) return KW_E_ARG;
  if (int rc = packed_dict(env->e, policies, npol, origin, out->dict)) return rc;
  out->exc_count = 0;
  BulkPass P(env, kb, policies, npol, origin, device, nullptr, (size_t)out->rows * npol, chunk_rows);
  P.pk = out;
  if (int rc = P.plan()) return rc;
  if (!P.chunked) return P.run_unchunked_packed();
  if (int rc = P.prepare()) return rc;
  int rc = P.setup();
  for (uint64_t k = 0; k < P.K && rc == KW_OK; ++k) rc = P.chunk(k);
  if (rc == KW_OK) rc = P.end_packed();
  return P.finish(rc);
}

int validate_host_summary(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, int device,
                          kw_summary* out, uint32_t chunk_rows) {
  if (!env || !kb || !out || !policies || npol == 0 || !out->col) return KW_E_ARG;
  if (env->e.device < 0 || !env->e.d_blob) return KW_E_DEVICE;
  if (device != env->e.device || out->rows != kb->b.n || out->npol != npol) return KW_E_ARG;
  BulkPass P(env, kb, policies, npol, origin, device, nullptr, (size_t)out->rows * npol, chunk_rows);
  P.sm = out;
  if (int rc = P.plan()) return rc;
  if (!P.chunked) return P.run_unchunked_summary();
  if (int rc = P.prepare()) return rc;
  int rc = P.setup();
  for (uint64_t k = 0; k < P.K && rc == KW_OK; ++k) rc = P.chunk(k);
  if (rc == KW_OK) rc = P.end_summary();
  return P.finish(rc);
}

}  // namespace kw
