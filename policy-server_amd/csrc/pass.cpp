// pass.cpp — a planned pass on a resident batch (pass.hpp): what its launches need on the device,
// the launches of the hot path (kernels.hip; plan.cpp plans it), verdict and side-data read-back.
#include "pass.hpp"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>

#include "groups.hpp"
#include "knobs.hpp"
#include "lastpass.hpp"
#include "plan.hpp"

namespace kw {

int upload_env(kw_env* env, int device) {
  if (device < 0) return KW_OK;
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipMalloc(&env->e.d_blob, env->e.blob.size()));
  HIPCHK(hipMemcpy(env->e.d_blob, env->e.blob.data(), env->e.blob.size(), hipMemcpyHostToDevice));
  env->e.device = device;
  return KW_OK;
}

int build_descs(const Batch& B, const TileArgs& T, uint64_t lo, uint64_t hi, uint64_t t0, uint64_t t1, uint64_t range,
                uint32_t grid, std::vector<TileDesc>* desc, std::vector<uint32_t>* ovf) {
  // descriptor of requests [r0, r1); false when it exceeds the capacities
  auto make = [&](uint64_t r0, uint64_t r1, TileDesc* dp) {
    TileDesc& d = *dp;
    memset(&d, 0, sizeof(d));
    d.r0lo = (uint32_t)r0;
    d.r0hi = (uint32_t)(r0 >> 32);
    d.nr = (uint32_t)(r1 - r0);
    d.cb = B.ctr_off[r0];
    d.ce = B.ctr_off[r1];
    d.lb = B.lbl_off[r0];
    d.le = B.lbl_off[r1];
    d.kab = B.capadd_off[d.cb];
    d.kae = B.capadd_off[d.ce];
    d.kdb = B.capdrop_off[d.cb];
    d.kde = B.capdrop_off[d.ce];
    bool fits = d.ce - d.cb <= T.cmax && d.kae - d.kab <= T.kmax && d.kde - d.kdb <= T.kmax && d.le - d.lb <= T.lmax;
    for (int m = 0; m < (int)NSTR; ++m) {
      if (!T.o_sb[m]) continue;
      uint64_t g0, g1;
      str_range(B, m, r0, r1, &g0, &g1);
      const StrCol& c = host_str(B, m);
      d.sa[m] = c.off[g0] & ~15u;
      d.nv[m] = (((c.off[g1] + 15u) & ~15u) - d.sa[m]) / 16u;
      fits = fits && d.nv[m] * 16u <= T.sb_cap[m];
    }
    d.fits = fits ? 1u : 0u;
    return fits;
  };
  // Block-aware cuts (KW_TILE_CUT, on by default): a tile from row r may end at any row of
  // [r + rows - rows / 8, r + rows], and ends where its estimated cost (kernels.hpp tile_cost) per
  // row is least, the longer tile on a tie: P1 and P2 pay per 64-item block, so a tile that stops
  // just before a segment spills into a nearly empty block does the same rows' work for a block
  // less. What is left of a range once it fits one tile stays one tile (two would pay the fixed
  // cost twice for no block saved). Off: every tile is `rows` tall, as before r08.
  // The choice is greedy, tile by tile, and each cut hands the rows it left out to the next tile, so
  // it is checked against the fixed cut twice. Per range: the cut descriptors are kept only where
  // their estimated cost sums to less than the fixed ones' (short tiles whose blocks are far from
  // full, 24-row ones for C4, gain nothing and pay the per-tile cost more often). Per call: the cuts
  // make ~2 % more tiles, and where that gives an XCD's busiest slot a tile more than the fixed cut
  // does (a launch of few tiles a slot, such as a small shard), a slot's extra tile costs more than
  // every tile's saved block; the fixed cut stays.
  // Not cut (profiles/r08_tile_cuts_ab.txt): launches of the image families alone (C2 / C3: no
  // block weights were fitted for them and the cuts measured +0.5 % at C2), and the bulk path's
  // per-chunk descriptors (grid 0: their build is on the pipeline's critical path, the cut build
  // costs 2-3 x the fixed one, and a chunk of whole rounds would not keep its cuts anyway).
  const bool cut = Knobs::on<KW_TILE_CUT>() && grid && (T.feat & (kFeatLbl | kFeatCtr));
  const TileCostW W = tile_cost_weights(T.feat, T.need);
  auto cost = [&](uint64_t r0, uint64_t r1) {
    const uint32_t cb = B.ctr_off[r0], ce = B.ctr_off[r1];
    return tile_cost(W, (uint32_t)(r1 - r0), B.lbl_off[r1] - B.lbl_off[r0], ce - cb,
                     (B.capadd_off[ce] - B.capadd_off[cb]) + (B.capdrop_off[ce] - B.capdrop_off[cb]));
  };
  const size_t nq = (size_t)((t1 - t0 + range - 1) / range);
  // [0]: the fixed cut, [1]: the block-aware one
  std::vector<std::vector<TileDesc>> qdesc[2] = {std::vector<std::vector<TileDesc>>(nq), std::vector<std::vector<TileDesc>>(nq)};
  std::vector<std::vector<uint32_t>> qovf[2] = {std::vector<std::vector<uint32_t>>(nq), std::vector<std::vector<uint32_t>>(nq)};
  std::vector<uint8_t> qcut(nq, 0);  // the range keeps its cut descriptors
  std::atomic<bool> too_far{false};
  HostWorkers::get().run(nq, [&](size_t q) {
    std::vector<std::pair<uint64_t, uint64_t>> todo;
    // the range's rows: the cuts are independent per range, so the ranges build in parallel and a
    // range's last tile is simply shorter
    const uint64_t qb = lo + (t0 + q * range) * T.rows;
    const uint64_t qe = std::min<uint64_t>(hi, lo + std::min<uint64_t>(t1, t0 + (q + 1) * range) * T.rows);
    uint64_t total[2] = {0, 0};
    for (int v = 0; v <= (cut ? 1 : 0); ++v) {
      std::vector<TileDesc>& dv = qdesc[v][q];
      dv.reserve((size_t)range + (v ? range / 8 : 0) + range / 64 + 1);
      for (uint64_t r = std::min(qb, qe); r < qe;) {
        uint64_t end = std::min<uint64_t>(qe, r + T.rows);
        if (v && end < qe) {
          uint64_t best = cost(r, end);
          for (uint64_t e = end - 1; e >= r + T.rows - T.rows / 8 && e > r; --e) {
            const uint64_t c = cost(r, e);
            if (c * (end - r) < best * (e - r)) best = c, end = e;  // c / (e - r) < best / (end - r)
          }
        }
        todo.assign(1, {r, end});
        r = end;
        while (!todo.empty()) {
          const auto [r0, r1] = todo.back();
          todo.pop_back();
          TileDesc d;
          if (make(r0, r1, &d)) {
            dv.push_back(d);
            total[v] += desc_cost(W, d);
          } else if (r1 - r0 > 1) {
            const uint64_t mid = r0 + (r1 - r0) / 2;
            todo.push_back({mid, r1});
            todo.push_back({r0, mid});
          } else {
            if (r0 > 0xffffffffull) too_far = true;  // overflow list holds u32 request indices
            qovf[v][q].push_back((uint32_t)r0);
          }
        }
      }
    }
    qcut[q] = cut && total[1] < total[0];
  });
  if (too_far) return KW_E_ARG;
  if (cut) {
    uint64_t n[2] = {0, 0};
    for (size_t q = 0; q < nq; ++q) n[0] += qdesc[0][q].size(), n[1] += qdesc[qcut[q]][q].size();
    auto rounds = [&](uint64_t nd) {  // tiles of the busiest slot (kernels.hpp tile_slot)
      uint64_t most = 0;
      for (uint32_t x = 0; x < tile_slot(nd, grid, 0).nx; ++x) {
        const TileSlot ts = tile_slot(nd, grid, x);
        most = std::max(most, (ts.t_hi - ts.t_lo + ts.wpx - 1) / ts.wpx);
      }
      return most;
    };
    if (rounds(n[1]) > rounds(n[0])) std::fill(qcut.begin(), qcut.end(), 0);
  }
  for (size_t q = 0; q < nq; ++q) {
    desc->insert(desc->end(), qdesc[qcut[q]][q].begin(), qdesc[qcut[q]][q].end());
    ovf->insert(ovf->end(), qovf[qcut[q]][q].begin(), qovf[qcut[q]][q].end());
  }
  return KW_OK;
}

uint64_t desc_cost(const TileCostW& w, const TileDesc& d) {
  return d.fits ? tile_cost(w, d.nr, d.le - d.lb, d.ce - d.cb, (d.kae - d.kab) + (d.kde - d.kdb)) : 0;
}

int plan_descs(const Batch& B, const PassPlan& plan, std::vector<TileDesc>* desc, std::vector<uint32_t>* ovf, uint64_t at[2],
               uint64_t nd[2]) {
  desc->clear();
  ovf->assign(1, 0u);
  if (plan.regions.size() > 2) return KW_E_ARG;
  for (size_t k = 0; k < plan.regions.size(); ++k) {  // region k's descriptors after region k-1's; one overflow list
    const PassPlan::Region& rg = plan.regions[k];
    const uint64_t ntiles = (rg.hi - rg.lo + rg.geom.rows - 1) / rg.geom.rows;
    at[k] = desc->size();
    desc->reserve(desc->size() + ntiles + ntiles / 8 + ntiles / 64 + 1);
    if (int rc = build_descs(B, rg.geom, rg.lo, rg.hi, 0, ntiles, 4096, rg.grid, desc, ovf)) return rc;
    nd[k] = desc->size() - at[k];
  }
  (*ovf)[0] = (uint32_t)(ovf->size() - 1);
  return KW_OK;
}

// Tile descriptors (kernels.hpp TileDesc) and the overflow list of one plan geometry, built from the
// host copy of the batch and uploaded once; reused while the geometry stays the same.
static int upload_tile_descs(const Batch& B, DeviceBatch* D, const PassPlan& plan, hipStream_t s) {
  uint64_t key = 1469598103934665603ull;
  auto mix = [&](uint64_t v) { key = (key ^ v) * 1099511628211ull; };
  mix(Knobs::on<KW_TILE_CUT>());
  for (const PassPlan::Region& rg : plan.regions) {
    const TileArgs& T = rg.geom;
    mix(rg.lo);
    mix(rg.hi);
    mix(rg.grid);  // the cuts are kept only where they cost this grid's busiest slot no tile more
    mix(T.feat);   // the cost weights
    mix(T.need);
    mix(T.rows);
    mix(T.cmax);
    mix(T.kmax);
    mix(T.lmax);
    for (int m = 0; m < (int)NSTR; ++m) {
      mix(T.o_sb[m] != 0);
      mix(T.sb_cap[m]);
    }
  }
  if (D->desc && D->desc_valid && key == D->desc_key) return KW_OK;
  const bool dbg = Knobs::on<KW_BULK_DEBUG>();  // diagnostics
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<TileDesc> desc;
  std::vector<uint32_t> ovf;
  uint64_t at[2] = {0, 0}, nd[2] = {0, 0};
  if (int rc = plan_descs(B, plan, &desc, &ovf, at, nd)) return rc;
  const auto t1 = std::chrono::steady_clock::now();
  HIPCHK(hipStreamSynchronize(s));  // a running pass may still read the previous descriptors
  D->h_desc = std::move(desc);
  D->h_ovf = std::move(ovf);
  if (int rc = ensure(&D->desc, &D->desc_cap, std::max<size_t>(D->h_desc.size(), 1))) return rc;
  if (int rc = ensure(&D->overflow, &D->overflow_cap, D->h_ovf.size())) return rc;
  if (!D->h_desc.empty())
    HIPCHK(hipMemcpyAsync(D->desc, D->h_desc.data(), D->h_desc.size() * sizeof(TileDesc), hipMemcpyHostToDevice, s));
  D->ndesc = D->h_desc.size();
  for (int k = 0; k < 2; ++k) {
    D->reg_desc[k] = at[k];
    D->reg_ndesc[k] = nd[k];
  }
  HIPCHK(hipMemcpyAsync(D->overflow, D->h_ovf.data(), D->h_ovf.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  D->n_overflow = D->h_ovf[0];
  D->desc_key = key;
  D->desc_valid = true;
  if (dbg)
    fprintf(stderr, "[kw descs] %zu descriptors: build %.2f ms, sync + upload %.2f ms\n", D->h_desc.size(),
            std::chrono::duration<double, std::milli>(t1 - t0).count(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
  return KW_OK;
}

int ensure_overflow_classes(const Batch& B, DeviceBatch* D, const TileArgs& T, EvalArgs* A) {
  const uint64_t nim = T.il.n(), nlv = std::max<uint32_t>(T.nlv, 1);
  const uint64_t n_ns = B.n + 1, n_ctr = B.containers() + 1, n_add = B.cap_add.n() + 1, n_drop = B.cap_drop.n() + 1,
                 n_lbl = B.labels() + 1;
  const uint64_t total = n_ns + n_ctr + n_ctr * std::max<uint64_t>(nim, 1) + n_add + n_drop + n_lbl + n_lbl * nlv;
  if (int rc = ensure(&D->g_cls, &D->g_cls_cap, (size_t)total)) return rc;
  uint16_t* p = D->g_cls;
  A->g_ns = p;
  p += n_ns;
  A->g_aa = p;
  p += n_ctr;
  A->g_img = p;
  p += n_ctr * std::max<uint64_t>(nim, 1);
  A->g_capadd = p;
  p += n_add;
  A->g_capdrop = p;
  p += n_drop;
  A->g_lk = (T.need & (1u << S_LK)) ? p : nullptr;
  p += n_lbl;
  A->g_lv = p;
  return KW_OK;
}

// NFA elements of a pass (kwdev.hpp DevNfa): the class arrays the tile kernel reads and the Pike
// VMs' scratch (nfa_classify_kernel, launched first by run_pass).
static int ensure_nfa(kw_batch* kb, PassPlan& plan, EvalArgs* A) {
  DeviceBatch& D = *kb->dev;
  const Batch& B = kb->b;
  const TileArgs& T = plan.geom;
  const DevHeader* H = (const DevHeader*)plan.env_blob;
  NfaPass& np = plan.nfa;
  memset(&np, 0, sizeof(np));
  np.nlv = T.nlv;
  np.nim = T.il.n();
  np.nlabels = B.labels();
  np.nctrs = B.containers();
  np.do_lv = (T.need & (1u << S_LV)) && (H->col[COL_LV].flags & 1u) && np.nlv ? 1u : 0u;
  np.do_img = (T.need & (1u << S_IMG)) && ((H->col[COL_REG].flags | H->col[COL_TAG].flags | H->col[COL_IMG].flags) & 1u) && np.nim
                  ? 1u
                  : 0u;
  if (np.do_img && D.max_image_len == 0xffffffffu) {
    uint32_t m = 0;
    for (uint64_t c = 0; c < B.containers(); ++c) m = std::max(m, B.ctr_image.off[c + 1] - B.ctr_image.off[c]);
    D.max_image_len = m;
  }
  np.nfa_words = H->nfa_words;
  np.subj_bytes = np.do_img ? ((D.max_image_len + 64u) & ~3u) : 0u;  // + "docker.io/library/" ":latest"
  np.words_per_thread = np.nfa_words + np.subj_bytes / 4u;
  const uint64_t nlv = std::max<uint32_t>(np.nlv, 1), nim = std::max<uint32_t>(np.nim, 1);
  const uint64_t n_lv = np.do_lv ? np.nlabels * nlv : 0, n_img = np.do_img ? np.nctrs * nim : 0;
  if (int rc = ensure(&D.nfa_cls, &D.nfa_cls_cap, (size_t)(n_lv + n_img + 1))) return rc;
  np.lv = D.nfa_cls;
  np.img = D.nfa_cls + n_lv;
  const uint64_t items = (np.do_lv ? np.nlabels : 0) + (np.do_img ? np.nctrs : 0);
  plan.nfa_threads = nfa_threads(items, np.words_per_thread);
  if (int rc = ensure(&D.nfa_scratch, &D.nfa_scratch_cap, (size_t)(plan.nfa_threads * np.words_per_thread + 1))) return rc;
  np.scratch = D.nfa_scratch;
  A->nfa_lv = np.do_lv ? np.lv : nullptr;
  A->nfa_img = np.do_img ? np.img : nullptr;
  return KW_OK;
}

int prepare_pass(kw_batch* kb, PassPlan& plan, hipStream_t s, EvalArgs* out_args, bool descs) {
  DeviceBatch& D = *kb->dev;
  const Batch& B = dev_rows(kb);
  if (D.cur && D.cur != s) HIPCHK(hipStreamSynchronize(D.cur));  // order against the previous pass's stream
  D.cur = s;
  // plan upload: records, per-launch TileArgs (with their record pointers), rows-mode column map
  if (int rc = ensure(&D.d_slots, &D.d_slots_cap, plan.slot_blob.size())) return rc;
  if (int rc = ensure(&D.d_tiles, &D.d_tiles_cap, plan.tiles.size())) return rc;
  for (size_t l = 0; l < plan.tiles.size(); ++l)
    for (uint32_t k = 0; k < plan.tiles[l].nchunk; ++k)
      plan.tiles[l].chunk[k].rec = D.d_slots + plan.slot_at[plan.launches[l % plan.launches.size()].first + k];
  if (D.h_slots != plan.slot_blob || D.h_tiles.size() != plan.tiles.size() ||
      (!plan.tiles.empty() && std::memcmp(D.h_tiles.data(), plan.tiles.data(), plan.tiles.size() * sizeof(TileArgs)) != 0)) {
    HIPCHK(hipStreamSynchronize(s));  // a running pass may still read the previous plan
    D.h_slots = plan.slot_blob;
    D.h_tiles = plan.tiles;
    HIPCHK(hipMemcpyAsync(D.d_slots, D.h_slots.data(), D.h_slots.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(D.d_tiles, D.h_tiles.data(), D.h_tiles.size() * sizeof(TileArgs), hipMemcpyHostToDevice, s));
  }
  EvalArgs A = plan.args;
  if (plan.rows_mode) {
    if (D.h_rowcol != plan.rowcol) {
      HIPCHK(hipStreamSynchronize(s));
      D.h_rowcol = plan.rowcol;
      if (int rc = ensure(&D.rowcol, &D.rowcol_cap, D.h_rowcol.size())) return rc;
      HIPCHK(hipMemcpyAsync(D.rowcol, D.h_rowcol.data(), D.h_rowcol.size() * 4, hipMemcpyHostToDevice, s));
    }
    A.rowcol = D.rowcol;
  }
  if (descs) {
    if (int rc = upload_tile_descs(B, &D, plan, s)) return rc;
  } else {  // the caller builds and uploads descriptors per row chunk (kw_validate_host)
    HIPCHK(hipStreamSynchronize(s));  // a running pass may still read the previous descriptors
    D.desc_valid = false;
    D.ndesc = 0;
    D.reg_ndesc[0] = D.reg_ndesc[1] = 0;
    D.n_overflow = 0;
  }
  A.ndesc = D.ndesc;
  // tests: KW_POISON_VERDICTS fills the verdict words with a sentinel no verdict word equals
  // (reason byte 0xA5) before the pass, so a tile the schedule never ran shows up as a mismatch
  // instead of keeping an earlier pass's words
  if (Knobs::on<KW_POISON_VERDICTS>())
    HIPCHK(hipMemsetAsync(D.verdicts, 0xA5, D.last_verdicts * sizeof(uint32_t), s));
  // the dynamic tile schedule's per-XCD counters (used by the regions whose plan says so,
  // sched_dynamic; run_pass hands them to those launches only)
  if (!D.sched) {
    void* p = nullptr;
    HIPCHK(dev_pool().alloc(D.device, 512 * sizeof(uint32_t), &p));
    D.sched = (uint32_t*)p;
    HIPCHK(hipMemsetAsync(D.sched, 0, 512 * sizeof(uint32_t), s));
  }
  A.sched = D.sched;
  A.sched_static = 2;  // run_pass chooses per launch (sched_static_rounds)
  // side data: dense group causes, the overflow path's class arrays and wide-argument list
  if (plan.nwide) {
    if (int rc = ensure(&D.wide_groups, &D.wide_groups_cap, (size_t)(B.n * plan.nwide))) return rc;
    A.wide_groups = D.wide_groups;
  }
  if (!D.wide_count) {
    void* p = nullptr;
    HIPCHK(dev_pool().alloc(D.device, sizeof(uint32_t), &p));
    D.wide_count = (uint32_t*)p;
  }
  // only the overflow kernels append wide records: a pass without overflow requests leaves the
  // counter alone (no fill launched between back-to-back passes) and has no records to read back
  D.wide_valid = D.n_overflow != 0;
  if (D.wide_valid) HIPCHK(hipMemsetAsync(D.wide_count, 0, sizeof(uint32_t), s));
  A.wide_count = D.wide_count;
  if (D.n_overflow) {
    if (int rc = ensure_overflow_classes(B, &D, plan.geom, &A)) return rc;
    const size_t cap = (size_t)D.n_overflow * plan.wide_cap_per_row;
    if (int rc = ensure(&D.wide_rec, &D.wide_rec_cap, cap)) return rc;
    A.wide_rec = D.wide_rec;
    A.wide_cap = (uint32_t)std::min<size_t>(cap, 0xffffffffu);
  }
  if (plan.geom.feat & kFeatNfa) {
    if (int rc = ensure_nfa(kb, plan, &A)) return rc;
  }
  D.last_nwide = plan.nwide;
  D.last_wide_policy = plan.wide_policy;
  D.last_rows_mode = plan.rows_mode;
  D.last_row_words = plan.args.npol;
  D.last_wide_cap = A.wide_cap;
  *out_args = A;
  return KW_OK;
}

// Diagnostics (KW_TILE_DEBUG & 512): the tile kernel's per-phase clocks of one launch, summed over
// its `grid` workgroups (ph: kPhaseWords words each). grid: the workgroups launched
// (tile_launch_grid), not the planner's count.
// ndesc, S: the launch's descriptors and static rounds (sched_static_rounds; -1: strided).
static void print_phase_report(size_t launch, uint32_t grid, const std::vector<uint64_t>& ph, uint64_t ndesc, int S) {
  double sum[kPhaseWords] = {0};
  for (uint32_t g = 0; g < grid; ++g)
    for (uint32_t k = 0; k < kPhaseWords; ++k) sum[k] += (double)ph[(size_t)g * kPhaseWords + k];
  const double tiles = std::max(1.0, sum[5]);
  fprintf(stderr,
          "[kw phase] launch %zu grid %u tiles %.0f: cycles/tile P0 %.0f P1 %.0f D %.0f P2 %.0f P3+next %.0f "
          "(sum %.0f); per workgroup: %.0f cycles, %.2f tiles, table staging %.0f\n",
          launch, grid, tiles, sum[0] / tiles, sum[1] / tiles, sum[2] / tiles, sum[3] / tiles, sum[4] / tiles,
          (sum[0] + sum[1] + sum[2] + sum[3] + sum[4]) / tiles, sum[6] / grid, tiles / grid, sum[7] / grid);
  // per wave and tile: P1 / P2 segment cycles, each phase's busy time and its barrier wait
  const double wt = tiles * (double)(kSlotThreads / 64u);
  const double* g = sum + 8;
  fprintf(stderr,
          "[kw seg] per wave-tile: P0 wait %.0f | P1 busy %.0f wait %.0f (label %.0f capstr %.0f ctr %.0f image %.0f req %.0f) "
          "| P2 busy %.0f wait %.0f (ctr %.0f label %.0f req %.0f) | P3 busy %.0f wait %.0f | P0 issue: top to fits %.0f "
          "job spans %.0f job loop %.0f\n",
          g[SG_P0_WAIT] / wt, g[SG_P1_BUSY] / wt, g[SG_P1_WAIT] / wt, g[SG_P1_LABEL] / wt, g[SG_P1_CAPSTR] / wt,
          g[SG_P1_CTR] / wt, g[SG_P1_IMAGE] / wt, g[SG_P1_REQ] / wt, g[SG_P2_BUSY] / wt, g[SG_P2_WAIT] / wt,
          g[SG_P2_CTR] / wt, g[SG_P2_LABEL] / wt, g[SG_P2_REQ] / wt, g[SG_P3_BUSY] / wt, g[SG_P3_WAIT] / wt,
          g[SG_P0_TOP] / wt, g[SG_P0_REQ] / wt, g[SG_P0_STR] / wt);
  // workgroup start times: a grid the CUs do not hold at once starts in waves. The real-time
  // counter is compared only within an XCD (workgroup b runs on XCD b % 8): the XCDs' counters
  // are not synchronised with each other.
  const uint32_t nx = std::min(8u, grid);
  uint32_t late = 0;
  double spread = 0;
  for (uint32_t x = 0; x < nx; ++x) {
    std::vector<uint64_t> st;
    for (uint32_t q = x; q < grid; q += nx) st.push_back(ph[(size_t)q * kPhaseWords + 8 + SG_START]);
    std::sort(st.begin(), st.end());
    for (uint64_t v : st) late += v > st[0] + 2000;  // > 20 us after the XCD's first
    spread = std::max(spread, (double)(st.back() - st[0]) / 100.0);
  }
  fprintf(stderr, "[kw start] launch %zu: %u of %u workgroups started > 20 us after their XCD's first (widest spread %.1f us)\n",
          launch, late, grid, spread);
  // workgroup end times, per XCD as above: the spread between the first and the last slot to finish,
  // and the share of slot-time (slots x the XCD's span from its first start to its last end) that
  // slots stand idle after their own end
  fprintf(stderr, "[kw finish] launch %zu: per XCD end spread us / idle share:", launch);
  double idle_all = 0, span_all = 0;
  uint32_t stamped = 0;
  for (uint32_t x = 0; x < nx; ++x) {
    uint64_t first = ~0ull, e_lo = ~0ull, e_hi = 0, n = 0, ends = 0;
    for (uint32_t q = x; q < grid; q += nx) {
      const uint64_t* w = &ph[(size_t)q * kPhaseWords + 8];
      if (!w[SG_START] || !w[SG_END]) continue;  // (a stamp that did not arrive)
      ++n;
      first = std::min(first, w[SG_START]);
      e_lo = std::min(e_lo, w[SG_END]);
      e_hi = std::max(e_hi, w[SG_END]);
      ends += w[SG_END];
    }
    const double idle = (double)n * (double)e_hi - (double)ends, span = (double)n * (double)(e_hi - first);
    idle_all += idle;
    span_all += span;
    stamped += (uint32_t)n;
    fprintf(stderr, " %.1f / %.1f %%", (double)(e_hi - e_lo) / 100.0, span > 0 ? 100.0 * idle / span : 0.0);
  }
  // (r08 saw a quarter of the start stamps read back zero "at grid 1024" and [kw start] count 768
  // late: the report then took the planner's grid, while the timing instantiation of C4 holds 3
  // workgroups a CU and launches 768. The zero stamps were workgroups that never ran. With the
  // launched grid every workgroup is stamped; the test above stays for a stamp that does not arrive.)
  fprintf(stderr, " (all: %.1f %% idle; %u of %u workgroups stamped)", span_all > 0 ? 100.0 * idle_all / span_all : 0.0,
          stamped, grid);
  // tiles run per workgroup: on the strided schedule the slots of an XCD differ by one at most, with a
  // counter-drawn tail the faster slots take more
  uint64_t t_min = ~0ull, t_max = 0;
  for (uint32_t q = 0; q < grid; ++q) {
    const uint64_t n = ph[(size_t)q * kPhaseWords + 5];
    t_min = std::min(t_min, n);
    t_max = std::max(t_max, n);
  }
  fprintf(stderr, "; tiles per workgroup min %llu mean %.2f max %llu", (unsigned long long)(grid ? t_min : 0), tiles / std::max(grid, 1u),
          (unsigned long long)t_max);
  if (S >= 0) {
    fprintf(stderr, "; S %d, tail tiles per XCD:", S);
    for (uint32_t x = 0; x < nx; ++x) {
      const TileSlot ts = tile_slot(ndesc, grid, x);
      fprintf(stderr, " %llu", (unsigned long long)(ts.t_hi - tile_tail_lo(ts, (uint32_t)S)));
    }
  }
  fprintf(stderr, "\n");
}

// One pass: prepare, the optional NFA pre-pass, the per-region launches, the overflow launch.
static int run_pass(kw_batch* kb, PassPlan& plan, bool timed, hipStream_t s) {
  DeviceBatch& D = *kb->dev;
  EvalArgs A;
  if (int rc = prepare_pass(kb, plan, s, &A)) return rc;
  // diagnostics: per-phase clocks of the tile kernel (KW_TILE_DEBUG & 512), printed per launch
  const bool phases = (plan.geom.debug & 512u) != 0;
  void* d_phase = nullptr;
  uint32_t gmax = 0;
  for (const PassPlan::Region& rg : plan.regions) gmax = std::max(gmax, rg.grid);
  const size_t phase_bytes = (size_t)gmax * kPhaseWords * sizeof(uint64_t);
  if (phases) {
    HIPCHK(hipMalloc(&d_phase, phase_bytes));
    A.phase = (uint64_t*)d_phase;
  }
  if (timed) HIPCHK(hipEventRecord(D.ev[0], s));
  if (plan.geom.feat & kFeatNfa) HIPCHK(launch_nfa_classify(A, D.d_tiles, plan.nfa, plan.nfa_threads, s));
  // region by region (a split batch: the light rows' launches, then the heavy rows'), each over its
  // own descriptors; the overflow kernels after the last region, over the one overflow list
  const size_t nl = plan.launches.size();
  D.last_launches.clear();
  D.last_kernels.clear();
  D.last_variants.clear();
  for (size_t l = 0; l < plan.tiles.size(); ++l) {
    const size_t k = l / nl;
    if (phases) HIPCHK(hipMemsetAsync(d_phase, 0, phase_bytes, s));
    // the workgroups the launch really runs: the kernel's schedule is in terms of gridDim.x, and the
    // planner's grid is clamped to what the device holds of this instantiation (the timing one runs
    // C4 at 3 workgroups a CU where the product kernel runs 4)
    const uint32_t grid = tile_launch_grid(plan.tiles[l], phases, plan.regions[k].grid);
    EvalArgs Ak = A;
    Ak.ndesc = D.reg_ndesc[k];
    // the schedule, from the launch's own descriptor count and grid: strided, or S static rounds and the counters
    const int S = sched_static_rounds(Ak.ndesc, grid, plan.regions[k].dyn);
    if (S < 0) Ak.sched = nullptr;
    else Ak.sched_static = (uint32_t)S;
    for (int64_t v : {(int64_t)grid, (int64_t)Ak.ndesc, (int64_t)S}) D.last_launches.push_back(v);
    D.last_kernels.push_back(tile_kernel_kind(plan.tiles[l], phases));
    D.last_variants.push_back(tile_variant_word(tile_variant(plan.tiles[l], phases)));
    HIPCHK(launch_evaluate_tiles(Ak, plan.tiles[l], D.d_tiles + l, D.desc + D.reg_desc[k], grid, s));
    if (phases) {
      std::vector<uint64_t> ph((size_t)grid * kPhaseWords);
      HIPCHK(hipMemcpyAsync(ph.data(), d_phase, ph.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      print_phase_report(l, grid, ph, Ak.ndesc, S);
    }
    if (D.n_overflow && k + 1 == plan.regions.size()) HIPCHK(launch_overflow(A, D.d_tiles + l, D.overflow, D.n_overflow, s));
  }
  if (timed) HIPCHK(hipEventRecord(D.ev[2], s));
  if (phases) HIPCHK(hipFree(d_phase));
  return KW_OK;
}

int run_validate(const kw_env* env, kw_batch* kb, PassPlan& plan, int origin, bool timed, hipStream_t s) {
  DeviceBatch& D = *kb->dev;
  const PassPlan::Wide& W = plan.wide;
  D.last_big_stride = 0;
  D.last_big_ref.clear();
  if (W.groups.empty()) return run_pass(kb, plan, timed, s);
  const uint64_t n = kb->b.n;
  const size_t nm = W.members.size();
  if (int rc = ensure(&D.member_words, &D.member_words_cap, (size_t)(n * nm))) return rc;
  {
    PassPlan mplan;
    if (int rc = plan_pass(env, kb, W.members.data(), (uint32_t)nm, nullptr, origin, Knobs::on<KW_BULK_DEBUG>(), &mplan)) return rc;
    mplan.args.out = D.member_words;
    if (int rc = run_pass(kb, mplan, false, s)) return rc;
  }
  if (int rc = run_pass(kb, plan, timed, s)) return rc;
  // combine: records (the groups', then the split members') | jump code | member maps in one upload
  const size_t g_bytes = (W.groups.size() + W.aux.size()) * sizeof(WideGroupArgs);
  const size_t p_at = g_bytes, m_at = (p_at + W.progs.size() + 15u) & ~(size_t)15u;
  const size_t bytes = m_at + W.midx.size() * 4;
  HIPCHK(hipStreamSynchronize(s));  // the upload buffer may still be read by the previous pass
  if (int rc = ensure(&D.wg_data, &D.wg_data_cap, bytes)) return rc;
  std::vector<uint8_t> h(bytes, 0);
  memcpy(h.data(), W.groups.data(), W.groups.size() * sizeof(WideGroupArgs));
  if (!W.aux.empty()) memcpy(h.data() + W.groups.size() * sizeof(WideGroupArgs), W.aux.data(), W.aux.size() * sizeof(WideGroupArgs));
  memcpy(h.data() + p_at, W.progs.data(), W.progs.size());
  memcpy(h.data() + m_at, W.midx.data(), W.midx.size() * 4);
  HIPCHK(hipMemcpyAsync(D.wg_data, h.data(), bytes, hipMemcpyHostToDevice, s));
  const uint64_t pairs = n * W.groups.size();
  const size_t stack_words = std::max<uint32_t>(W.stack_words, 1);
  // (a script that builds strings or arrays carries a 16 KB arena per thread: the grid keeps the
  // scratch under 1 GiB; every thread loops over its pairs)
  const uint64_t max_grid = std::max<uint64_t>(1, (1ull << 30) / (256ull * 8ull * stack_words));
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(pairs + 255) / 256, 1024, max_grid}));
  if (int rc = ensure(&D.wg_stack, &D.wg_stack_cap, (size_t)grid * 256 * stack_words)) return rc;
  if (int rc = ensure(&D.big_causes, &D.big_causes_cap, (size_t)(n * W.cause_stride))) return rc;
  HIPCHK(hipMemsetAsync(D.big_causes, 0, (size_t)(n * W.cause_stride) * 8, s));
  WideGroupPass w;
  memset(&w, 0, sizeof(w));
  w.groups = (const WideGroupArgs*)D.wg_data;
  w.ngroups = (uint32_t)W.groups.size();
  w.progs = D.wg_data + p_at;
  w.midx = (const uint32_t*)(D.wg_data + m_at);
  w.member_words = D.member_words;
  w.nmw = (uint32_t)nm;
  w.out = D.verdicts;
  w.npol = plan.args.npol;
  w.rowcol = plan.rows_mode ? D.rowcol : nullptr;
  w.causes = D.big_causes;
  w.cause_stride = W.cause_stride;
  w.stack = D.wg_stack;
  w.stack_words = (uint32_t)stack_words;
  w.nrows = n;
  HIPCHK(launch_wide_groups(w, grid, s));
  D.last_big_stride = W.cause_stride;
  for (size_t k = 0; k < W.groups.size(); ++k)
    D.last_big_ref.push_back({W.policy[k], W.groups[k].cause_off, W.groups[k].cause_words});
  HIPCHK(hipStreamSynchronize(s));  // the host copy `h` is freed on return
  return KW_OK;
}

int validate_common(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, const int32_t* row_policy,
                    int origin, PassPlan* plan) {
  if (!env || !kb) return KW_E_ARG;
  const Env& E = env->e;
  if (E.device < 0 || !E.d_blob) return KW_E_DEVICE;  // no silent host fallback: the hot path is the GPU
  if (!kb->dev) return KW_E_ARG;                        // batch not resident
  if (kb->dev->device != E.device) return KW_E_ARG;
  if (origin != KW_ORIGIN_VALIDATE && origin != KW_ORIGIN_AUDIT) return KW_E_ARG;
  DeviceBatch& D = *kb->dev;
  HIPCHK(hipSetDevice(D.device));
  const int32_t np = (int32_t)E.nvisible;  // (the hidden parts of split policies are not addressable)
  uint64_t npairs;
  if (row_policy) {
    for (uint64_t r = 0; r < kb->b.n; ++r)
      if (row_policy[r] < 0 || row_policy[r] >= np) return KW_E_ARG;
    npairs = kb->b.n;
  } else {
    if (npol == 0 || !policies) return KW_E_ARG;
    for (uint32_t j = 0; j < npol; ++j)
      if (policies[j] < 0 || policies[j] >= np) return KW_E_ARG;
    npairs = kb->b.n * (uint64_t)npol;
  }
  if (int rc = ensure(&D.verdicts, &D.verdict_cap, npairs)) return rc;
  D.last_verdicts = npairs;
  kb->b.wide.clear();
  if (int rc = plan_pass(env, kb, policies, npol, row_policy, origin, Knobs::on<KW_BULK_DEBUG>(), plan)) return rc;
  return (plan->geom.need & ~D.loaded) ? KW_E_ARG : KW_OK;  // a column the upload left out (kw_validate_host)
}

int validate_cached(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, PassPlan** out) {
  DeviceBatch* D = kb && kb->dev ? kb->dev.get() : nullptr;
  const uint64_t knobs = kw_knob_hash();
  if (env && D && D->plan_cache && D->plan_env == env->uid && D->plan_origin == origin && D->plan_knobs == knobs &&
      D->plan_pols.size() == npol && policies && std::equal(policies, policies + npol, D->plan_pols.begin())) {
    PassPlan* plan = D->plan_cache.get();
    const Env& E = env->e;
    if (E.device < 0 || !E.d_blob) return KW_E_DEVICE;
    if (D->device != E.device) return KW_E_ARG;
    HIPCHK(hipSetDevice(D->device));
    const uint64_t npairs = kb->b.n * (uint64_t)npol;
    uint32_t* before = D->verdicts;
    if (int rc = ensure(&D->verdicts, &D->verdict_cap, npairs)) return rc;
    if (D->verdicts != before) {  // (reallocated by another pass's larger need: re-plan)
      D->plan_cache.reset();
      return validate_cached(env, kb, policies, npol, origin, out);
    }
    D->last_verdicts = npairs;
    kb->b.wide.clear();
    if (plan->geom.need & ~D->loaded) return KW_E_ARG;
    *out = plan;
    return KW_OK;
  }
  auto plan = std::make_shared<PassPlan>();
  if (D) D->plan_cache.reset();
  if (int rc = validate_common(env, kb, policies, npol, nullptr, origin, plan.get())) return rc;
  D = kb->dev.get();
  D->plan_cache = plan;
  D->plan_env = env->uid;
  D->plan_origin = origin;
  D->plan_knobs = knobs;
  D->plan_pols.assign(policies, policies + npol);
  *out = plan.get();
  return KW_OK;
}

int validate_timed(const kw_env* env, kw_batch* b, const int32_t* policies, uint32_t npol, int origin, int warmup, int reps,
                   kw_timing* out) {
  if (!out || reps <= 0) return KW_E_ARG;
  PassPlan plan;
  if (int rc = validate_common(env, b, policies, npol, nullptr, origin, &plan)) return rc;
  DeviceBatch& D = *b->dev;
  for (auto& e : D.ev)
    if (!e) HIPCHK(hipEventCreate(&e));
  for (int i = 0; i < warmup; ++i)
    if (int rc = run_validate(env, b, plan, origin, false, D.stream)) return rc;
  HIPCHK(hipStreamSynchronize(D.stream));
  double ev = 0;
  for (int i = 0; i < reps; ++i) {
    if (int rc = run_validate(env, b, plan, origin, true, D.stream)) return rc;
    HIPCHK(hipEventSynchronize(D.ev[2]));
    float c = 0;
    HIPCHK(hipEventElapsedTime(&c, D.ev[0], D.ev[2]));
    ev += c;
  }
  out->classify_ms = 0;
  out->evaluate_ms = ev / reps;
  out->total_ms = ev / reps;
  out->classify_bytes = 0;
  out->evaluate_bytes = plan.evaluate_bytes;
  return KW_OK;
}

int load_side_data(kw_batch* b, hipStream_t s) {
  DeviceBatch& D = *b->dev;
  WideData& W = b->b.wide;
  W.clear();
  uint32_t nrec = 0;
  if (D.wide_count && D.wide_valid) HIPCHK(hipMemcpyAsync(&nrec, D.wide_count, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  W.nwide = D.last_nwide;
  W.wide_policy = D.last_wide_policy;
  W.rows_mode = D.last_rows_mode;
  if (D.last_big_stride && D.big_causes) {  // wide-group cause bitsets
    W.big_stride = D.last_big_stride;
    W.big_ref = D.last_big_ref;
    W.big.resize(b->b.n * W.big_stride);
    if (!W.big.empty()) HIPCHK(hipMemcpyAsync(W.big.data(), D.big_causes, W.big.size() * 8, hipMemcpyDeviceToHost, s));
  }
  if (W.nwide) {
    W.groups.resize(b->b.n * W.nwide);
    if (!W.groups.empty())
      HIPCHK(hipMemcpyAsync(W.groups.data(), D.wide_groups, W.groups.size() * 8, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  if (D.split) {  // device-row order (light / heavy split) -> batch rows
    auto unperm = [&](std::vector<uint64_t>* v, uint32_t stride) {
      if (v->empty() || !stride) return;
      std::vector<uint64_t> t(v->size());
      for (uint64_t d = 0; d < b->b.n; ++d)
        std::copy_n(v->data() + d * stride, stride, t.data() + D.perm[d] * stride);
      v->swap(t);
    };
    unperm(&W.big, W.big_stride);
    unperm(&W.groups, W.nwide);
  }
  nrec = std::min(nrec, D.last_wide_cap);
  if (nrec) {
    std::vector<WideRec> rec(nrec);
    HIPCHK(hipMemcpy(rec.data(), D.wide_rec, nrec * sizeof(WideRec), hipMemcpyDeviceToHost));
    for (const WideRec& r : rec) {
      const uint64_t d = (uint64_t)r.row_lo | ((uint64_t)r.row_hi << 32);
      W.recs.push_back({D.split ? D.perm[d] : d, (int32_t)r.policy, r.value});
    }
    std::sort(W.recs.begin(), W.recs.end(), [](const WideData::Rec& x, const WideData::Rec& y) {
      return x.row < y.row || (x.row == y.row && x.policy < y.policy);
    });
  }
  return KW_OK;
}

int read_verdicts(kw_batch* b, uint32_t* host_out, size_t count) {
  if (!b || !b->dev || (!host_out && count)) return KW_E_ARG;
  DeviceBatch& D = *b->dev;
  if (count > D.last_verdicts) return KW_E_ARG;
  HIPCHK(hipSetDevice(D.device));
  hipStream_t s = D.cur ? D.cur : D.stream;
  const size_t vbytes = count * sizeof(uint32_t);
  {
    // (the bounce block returns to the pool on the error returns too: each one precedes the
    // enqueue or follows a failed enqueue or synchronise)
    BlockLease bounce;
    if (D.split && count) {
      // rows in device order (light / heavy split): whole device rows through a pinned bounce block,
      // each scattered to its batch row's words below `count`
      const uint64_t rw = std::max<uint32_t>(D.last_row_words, 1), nrows = D.last_verdicts / rw;
      const uint64_t per = std::max<uint64_t>(1, kBounce / (rw * 4));
      HIPCHK(bounce.alloc(host_pool(), D.device, kBounce));
      for (uint64_t d0 = 0; d0 < nrows; d0 += per) {
        const uint64_t d1 = std::min(nrows, d0 + per);
        HIPCHK(hipMemcpyAsync(bounce.p, D.verdicts + d0 * rw, (d1 - d0) * rw * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const uint32_t* src = (const uint32_t*)bounce.p;
        HostWorkers::get().run((size_t)((d1 - d0 + 4095) / 4096), [&](size_t q) {
          for (uint64_t d = d0 + q * 4096, e = std::min(d1, d0 + (q + 1) * 4096); d < e; ++d) {
            const uint64_t w0 = D.perm[d] * rw;
            if (w0 < count) memcpy(host_out + w0, src + (d - d0) * rw, std::min<uint64_t>(rw, count - w0) * 4);
          }
        });
      }
    } else if (vbytes > ((size_t)16 << 20)) {
      // large read-backs through a pinned bounce block (full-rate DMA), fanned out to the caller's
      // (pageable) buffer by several threads
      if (int rc = bounce_read(bounce, D.device, s, host_out, D.verdicts, vbytes)) return rc;
    } else if (count) {
      HIPCHK(hipMemcpyAsync(host_out, D.verdicts, vbytes, hipMemcpyDeviceToHost, s));
    }
  }
  return load_side_data(b, s);
}

}  // namespace kw
