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
//   read_back      sc: the output form's kernels over the chunk's rows of the verdict buffer (reduce;
//                  the words form has none), records ev[3k+1]; s_out: waits ev[3k+1], the form's D2H
//                  copies of the chunk (copies), records ev[3k+2]
//   landed(k-1)    the form's host side of chunk k-1, behind its host wait for ev[3(k-1)+2]
// and after the last chunk the form's end() (landed(K-1) and what closes the form), then the drain of
// s_in, sc, s_out — on every path, errors included — before any block, stream or event returns to
// its pool (Res). What reduce, copies, landed and end do in each form, and the events the packed form
// owns beyond these, stands with the forms in bulkout.hpp. The packed and the summary form of a pass
// that ran unchunked go through its verdict buffer in row slabs by the same read_back / landed / end.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <optional>

#include "bulkout.hpp"
#include "bulkplan.hpp"
#include "knobs.hpp"
#include "packed.hpp"
#include "pass.hpp"
#include "plan.hpp"
#include "upload.hpp"

namespace kw {
namespace {

// staged columns: each chunk's ranges packed into one pinned slot, one H2D into the device slot,
// then the scatter kernel puts them in place (one copy per chunk, not one per column). kRing
// slots: packing chunk k waits for chunk k - kRing's upload. KW_BULK_PACK=0: a copy per column
// range (A/B knob, profiles/r05_bulk_copies.txt).
constexpr uint64_t kRing = 4;

// What a chunked pass takes from the pools for the length of the call. The destructor drains the
// three streams; the leases are members, so they return to their pools after it on every path: a
// block returned while a copy into it is in flight would be handed to another thread's pass.
struct Res {
  hipStream_t sc;
  BlockLease dland, hpack;  // the landing ring on the device and the pack ring in pinned memory
  BlockLease hdesc;         // the pinned descriptor halves
  OutBlocks blk;            // the output form's blocks
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
  BulkOut& form;  // what becomes of the verdict words
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
  std::vector<uint64_t> tb, rb;  // chunk k: tiles [tb[k], tb[k+1]), rows [rb[k], rb[k+1])
  uint64_t K = 0, depth = 0, dcap = 0;
  bool pinned = false, packed = false;
  size_t slot_bytes = 0;
  std::optional<Res> res;
  // per chunk: its descriptors and overflow list; overflow requests so far
  std::vector<TileDesc> cd;
  std::vector<uint32_t> co;
  uint64_t n_ovf = 0;

  BulkPass(const kw_env* e, kw_batch* b, const int32_t* p, uint32_t np, int o, int dev, BulkOut& f, uint32_t cr)
      : env(e), kb(b), policies(p), npol(np), origin(o), device(dev), form(f), chunk_rows(cr) {}

  uint64_t row_of(uint64_t tile) const { return std::min<uint64_t>(kb->b.n, tile * pl.geom.rows); }
  uint64_t per_rows() const { return chunk_rows ? chunk_rows : (uint64_t)Knobs::num<KW_BULK_CHUNK>(); }  // A/B knob (profiles/r04_bulk_sweep.txt)
  BulkCtx ctx() { return {res->blk, sc, res->s_out.s, res->ev, kb->dev->verdicts, device, npol, kb->b.n, K, rb, pinned, t}; }

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
      piece_range(kb->b, p, rb[k], rb[k + 1], k + 1 == K, &lo, &hi);
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

  // One upload, the full pass; then one read-back, or the form goes through the verdict buffer in
  // row slabs by the chunked pass's steps.
  int run_unchunked() {
    if (int rc = run_whole()) return rc;
    if (!form.in_slabs()) return form.whole(kb);
    rb = slab_bounds(kb->b.n, per_rows());
    K = rb.size() - 1;
    if (K == 0) {
      form.empty();
      return load_side_data(kb, sc);
    }
    pinned = Knobs::on<KW_BULK_DIRECT>() && form.direct();
    res.emplace(sc);
    int rc = form.setup(ctx(), rb[1]);  // (the first slab is the largest)
    if (rc == KW_OK && (res->s_out.get(device) != hipSuccess || res->ev.get(device, form.events_per_chunk() * K) != hipSuccess))
      rc = KW_E_DEVICE;
    for (uint64_t k = 0; k < K && rc == KW_OK; ++k) {
      rc = read_back(k);
      if (rc == KW_OK && k >= 1) rc = form.landed(ctx(), k - 1);
    }
    if (rc == KW_OK) rc = form.end(ctx());
    res->drain();
    res.reset();
    if (rc != KW_OK && !form.tolerates(rc)) return rc;
    const int src = load_side_data(kb, sc);
    return src ? src : rc;
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

  // The chunk schedule and what the chunks share: the form's blocks, descriptor halves, the packed
  // ring, streams and events. From here on a failure leaves the batch's columns partly uploaded
  // (finish clears D.loaded).
  int setup() {
    const TileArgs& G = pl.geom;
    const uint64_t ntiles = (kb->b.n + G.rows - 1) / G.rows;
    const uint64_t per = per_rows();
    const bool ramp = Knobs::on<KW_BULK_RAMP>();  // A/B knob
    const uint64_t tper = chunk_tiles(ntiles, G.rows, per);
    tb = chunk_bounds(ntiles, G.rows, per, ramp);
    K = tb.size() - 1;
    for (uint64_t k = 0; k <= K; ++k) rb.push_back(row_of(tb[k]));
    pinned = Knobs::on<KW_BULK_DIRECT>() && form.direct();  // A/B knob
    const int depth_knob = Knobs::num<KW_BULK_DEPTH>();     // A/B knob, 0 = unbounded
    depth = bulk_depth(depth_knob, std::count(dma.begin(), dma.end(), 1) > 0);
    // (the largest chunk: `per` grows past ~240 chunks)
    uint64_t max_rows = 0;
    for (uint64_t k = 0; k < K; ++k) max_rows = std::max(max_rows, rb[k + 1] - rb[k]);
    dcap = tper + tper / 4 + 64;
    res.emplace(sc);
    if (int rc = form.setup(ctx(), max_rows)) return rc;
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
    HIPCHK(res->ev.get(device, form.events_per_chunk() * K));
    return KW_OK;
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

  // The form's kernels behind the chunk's on sc; its copies on s_out between ev[3k+1] and ev[3k+2].
  int read_back(uint64_t k) {
    const BulkCtx c = ctx();
    if (int rc = form.reduce(c, k)) return rc;
    HIPCHK(hipEventRecord(c.ev[3 * k + 1], sc));
    HIPCHK(hipStreamWaitEvent(c.s_out, c.ev[3 * k + 1], 0));
    if (int rc = form.copies(c, k)) return rc;
    HIPCHK(hipEventRecord(c.ev[3 * k + 2], c.s_out));
    return KW_OK;
  }

  int chunk(uint64_t k) {
    if (int rc = stage_columns(k)) return rc;
    if (int rc = stage_descs(k)) return rc;
    const auto t2 = clk::now();
    if (int rc = launch(k)) return rc;
    if (co[0])
      if (int rc = overflow()) return rc;
    if (int rc = read_back(k)) return rc;
    t.enq += since(t2);
    if (k == 0) t.first = since(t_start);
    return k >= 1 ? form.landed(ctx(), k - 1) : KW_OK;
  }

  // plan, then the pass unchunked, or chunk by chunk; the form's end; finish.
  int run() {
    if (int rc = plan()) return rc;
    if (!chunked) return run_unchunked();
    if (int rc = prepare()) return rc;
    int rc = setup();
    for (uint64_t k = 0; k < K && rc == KW_OK; ++k) rc = chunk(k);
    if (rc == KW_OK) rc = form.end(ctx());
    return finish(rc);
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
    if (rc != KW_OK && !form.tolerates(rc)) {
      D.loaded = 0;
      return rc;
    }
    if (int src = load_side_data(kb, sc)) rc = src;  // overflow requests' wide arguments (kw_batch_wide_arg)
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
  WordsOut form(out, count);
  return BulkPass(env, kb, policies, npol, origin, device, form, chunk_rows).run();
}

int validate_host_packed(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, int device,
                         kw_packed* out, uint32_t chunk_rows) {
  if (!env || !kb || !out || !policies || npol == 0) return KW_E_ARG;
  if (env->e.device < 0 || !env->e.d_blob) return KW_E_DEVICE;
  if (device != env->e.device || out->rows != kb->b.n || out->npol != npol || !packed_fits(out->rows, npol)) return KW_E_ARG;
  if (!out->dict || !out->exc_off || (out->rows && !out->planes) || (out->exc_cap && !out->exc)) return KW_E_ARG;
  if (int rc = packed_dict(env->e, policies, npol, origin, out->dict)) return rc;
  out->exc_count = 0;
  PackedOut form(out);
  return BulkPass(env, kb, policies, npol, origin, device, form, chunk_rows).run();
}

int validate_host_summary(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, int device,
                          kw_summary* out, uint32_t chunk_rows) {
  if (!env || !kb || !out || !policies || npol == 0 || !out->col) return KW_E_ARG;
  if (env->e.device < 0 || !env->e.d_blob) return KW_E_DEVICE;
  if (device != env->e.device || out->rows != kb->b.n || out->npol != npol) return KW_E_ARG;
  SummaryOut form(out);
  return BulkPass(env, kb, policies, npol, origin, device, form, chunk_rows).run();
}

}  // namespace kw
