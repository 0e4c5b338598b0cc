// capi.cpp — extern "C" implementation of include/kwgpu.h: environment and batch lifetime, HBM
// residency, launch of the hot path (kernels.hip; plan.cpp plans it) and the host epilogue (service.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/kwgpu.h"
#include "automaton.hpp"
#include "batch.hpp"
#include "devbatch.hpp"
#include "env.hpp"
#include "kernels.hpp"
#include "knobs.hpp"
#include "metrics.hpp"
#include "plan.hpp"
#include "pools.hpp"
#include "service.hpp"
#include "slotplan.hpp"
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

#define HIPCHK(x)                             \
  do {                                        \
    hipError_t _e = (x);                      \
    if (_e != hipSuccess) return KW_E_DEVICE; \
  } while (0)

// Device buffer of at least n elements from the pool (the current device's), replacing a smaller one.
template <typename T>
int ensure(T** p, size_t* cap, size_t n) {
  if (*cap >= n && *p) return KW_OK;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  dev_pool().release(dev, *p, *cap * sizeof(T));
  *p = nullptr;
  const size_t want = BlockPool::cls(std::max<size_t>(n, 1) * sizeof(T)) / sizeof(T);
  void* q = nullptr;
  HIPCHK(dev_pool().alloc(dev, want * sizeof(T), &q));
  *p = (T*)q;
  *cap = want;
  return KW_OK;
}

int upload_env(kw_env* env, int device) {
  if (device < 0) return KW_OK;
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipMalloc(&env->e.d_blob, env->e.blob.size()));
  HIPCHK(hipMemcpy(env->e.d_blob, env->e.blob.data(), env->e.blob.size(), hipMemcpyHostToDevice));
  env->e.device = device;
  return KW_OK;
}

// Tile descriptors (kernels.hpp TileDesc) and the overflow list of one plan geometry, built from the
// host copy of the batch and uploaded once; reused while the geometry stays the same.
// The descriptors of tiles [t0, t1) of geometry T over rows [lo, hi), in row order, and the requests that exceed the
// capacities alone (overflow); a run that does not fit is halved until its parts do. Tiles in ranges
// of `range` on the host workers. KW_E_ARG when an overflow request index exceeds u32.
int build_descs(const Batch& B, const TileArgs& T, uint64_t lo, uint64_t hi, uint64_t t0, uint64_t t1, uint64_t range,
                std::vector<TileDesc>* desc, std::vector<uint32_t>* ovf) {
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
  const size_t nq = (size_t)((t1 - t0 + range - 1) / range);
  std::vector<std::vector<TileDesc>> qdesc(nq);
  std::vector<std::vector<uint32_t>> qovf(nq);
  std::atomic<bool> too_far{false};
  HostWorkers::get().run(nq, [&](size_t q) {
    std::vector<std::pair<uint64_t, uint64_t>> todo;
    std::vector<TileDesc>& dv = qdesc[q];
    dv.reserve((size_t)range + range / 64);
    for (uint64_t tile = t0 + q * range, te = std::min<uint64_t>(t1, t0 + (q + 1) * range); tile < te; ++tile) {
      todo.assign(1, {lo + tile * T.rows, std::min<uint64_t>(hi, lo + (tile + 1) * T.rows)});
      while (!todo.empty()) {
        const auto [r0, r1] = todo.back();
        todo.pop_back();
        TileDesc d;
        if (make(r0, r1, &d)) {
          dv.push_back(d);
        } else if (r1 - r0 > 1) {
          const uint64_t mid = r0 + (r1 - r0) / 2;
          todo.push_back({mid, r1});
          todo.push_back({r0, mid});
        } else {
          if (r0 > 0xffffffffull) too_far = true;  // overflow list holds u32 request indices
          qovf[q].push_back((uint32_t)r0);
        }
      }
    }
  });
  if (too_far) return KW_E_ARG;
  for (size_t q = 0; q < nq; ++q) {
    desc->insert(desc->end(), qdesc[q].begin(), qdesc[q].end());
    ovf->insert(ovf->end(), qovf[q].begin(), qovf[q].end());
  }
  return KW_OK;
}

int upload_tile_descs(const Batch& B, DeviceBatch* D, const PassPlan& plan, hipStream_t s) {
  uint64_t key = 1469598103934665603ull;
  auto mix = [&](uint64_t v) { key = (key ^ v) * 1099511628211ull; };
  for (const PassPlan::Region& rg : plan.regions) {
    const TileArgs& T = rg.geom;
    mix(rg.lo);
    mix(rg.hi);
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
  std::vector<uint32_t> ovf{0};
  if (plan.regions.size() > 2) return KW_E_ARG;
  uint64_t at[2] = {0, 0}, nd[2] = {0, 0};
  for (size_t k = 0; k < plan.regions.size(); ++k) {  // region k's descriptors after region k-1's; one overflow list
    const PassPlan::Region& rg = plan.regions[k];
    const uint64_t ntiles = (rg.hi - rg.lo + rg.geom.rows - 1) / rg.geom.rows;
    at[k] = desc.size();
    desc.reserve(desc.size() + ntiles + ntiles / 64 + 1);
    if (int rc = build_descs(B, rg.geom, rg.lo, rg.hi, 0, ntiles, 4096, &desc, &ovf)) return rc;
    nd[k] = desc.size() - at[k];
  }
  ovf[0] = (uint32_t)(ovf.size() - 1);
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

// Per-string class arrays of the overflow path (absolute entity indices), one allocation.
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
int ensure_nfa(kw_batch* kb, PassPlan& plan, EvalArgs* A) {
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

// Everything a pass's launches need on the device before the first one: the plan's records and
// TileArgs, the rows-mode column map, tile descriptors and overflow list, schedule counters and the
// side-data buffers; *out_args: the launch arguments.
int prepare_pass(kw_batch* kb, PassPlan& plan, hipStream_t s, EvalArgs* out_args, bool descs = true) {
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

int run_pass(kw_batch* kb, PassPlan& plan, bool timed, hipStream_t s) {
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
  for (size_t l = 0; l < plan.tiles.size(); ++l) {
    const size_t k = l / nl;
    if (phases) HIPCHK(hipMemsetAsync(d_phase, 0, phase_bytes, s));
    const uint32_t grid = plan.regions[k].grid;
    EvalArgs Ak = A;
    Ak.ndesc = D.reg_ndesc[k];
    if (!plan.regions[k].dyn) Ak.sched = nullptr;  // the strided schedule
    HIPCHK(launch_evaluate_tiles(Ak, plan.tiles[l], D.d_tiles + l, D.desc + D.reg_desc[k], grid, s));
    if (phases) {
      std::vector<uint64_t> ph((size_t)grid * kPhaseWords);
      HIPCHK(hipMemcpyAsync(ph.data(), d_phase, ph.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      double sum[kPhaseWords] = {0};
      for (uint32_t g = 0; g < grid; ++g)
        for (uint32_t k = 0; k < kPhaseWords; ++k) sum[k] += (double)ph[(size_t)g * kPhaseWords + k];
      const double tiles = std::max(1.0, sum[5]);
      fprintf(stderr,
              "[kw phase] launch %zu grid %u tiles %.0f: cycles/tile P0 %.0f P1 %.0f D %.0f P2 %.0f P3+next %.0f "
              "(sum %.0f); per workgroup: %.0f cycles, %.2f tiles, table staging %.0f\n",
              l, grid, tiles, sum[0] / tiles, sum[1] / tiles, sum[2] / tiles, sum[3] / tiles, sum[4] / tiles,
              (sum[0] + sum[1] + sum[2] + sum[3] + sum[4]) / tiles, sum[6] / grid, tiles / grid, sum[7] / grid);
      // per wave and tile: P1 / P2 segment cycles, each phase's busy time and its barrier wait
      const double wt = tiles * (double)(kSlotThreads / 64u);
      const double* g = sum + 8;
      fprintf(stderr,
              "[kw seg] per wave-tile: P0 wait %.0f | P1 busy %.0f wait %.0f (label %.0f capstr %.0f ctr %.0f image %.0f req %.0f) "
              "| P2 busy %.0f wait %.0f (ctr %.0f label %.0f req %.0f) | P3 busy %.0f wait %.0f | P0 issue: top %.0f "
              "request arrays %.0f strings %.0f\n",
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
              l, late, grid, spread);
    }
    if (D.n_overflow && k + 1 == plan.regions.size()) HIPCHK(launch_overflow(A, D.d_tiles + l, D.overflow, D.n_overflow, s));
  }
  if (timed) HIPCHK(hipEventRecord(D.ev[2], s));
  if (phases) HIPCHK(hipFree(d_phase));
  return KW_OK;
}

// A planned pass with its wide policy groups (PassPlan::wide): their members first run as a
// separate all-pairs pass into member_words, then the pass itself (wide columns hold a
// placeholder), then the combine kernel writes those columns and their cause bitsets. The member
// pass's own side data (entity indices >= 65535 of members) is not kept: the main pass reuses the
// buffers. `timed`: HIP events bracket the main pass.
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

// validate_common for an all-pairs pass through the batch's plan cache (DeviceBatch::plan_cache):
// a repeated pass (same environment, policy list, origin and KW_* settings) skips planning; the
// checks and the verdict buffer are redone every time.
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

}  // extern "C"

namespace {
// Upload the batch's columns to `device`: one pooled allocation with 256-B aligned sub-arrays,
// assembled in pinned host staging and copied with one async H2D on `stream` (null: a new stream
// owned by the batch); `sync` waits for the copy.
// A column of the device batch image: where its bytes come from and sit, and how a row range maps
// onto it (the bulk path uploads row chunks separately).
enum PieceKind { PK_ROW_U8, PK_ROW_OFF, PK_CTR_U8, PK_CTR_OFF, PK_STR_OFF, PK_STR_BYTES };
struct Piece {
  const void* src;
  size_t bytes;  // source bytes (reserved 256-B aligned in the image)
  size_t at;     // offset in the device image and in the pinned staging
  PieceKind kind;
  int m;         // string column (PK_STR_*), else -1
  bool gather;   // string bytes of a reordered batch (gather_column), src null
};

// Allocates the batch's device image (one pooled allocation, 256-B aligned sub-arrays) and its
// pinned staging block, and points the DeviceBatch views at it; nothing is copied.
// ---- light / heavy split at upload. A batch whose container counts
// are heavy-tailed (C5: Zipf over 1..64 — 14.7 % of the requests hold 63 % of the containers) sizes
// every tile's capacities, and so the occupancy, by the heavy requests scattered through it. The
// device copy instead holds the light requests (<= KW_HEAVY_CTR containers, 5) first and the heavy
// ones after them, in batch order within each region; the planner gives each region its own tile
// geometry (plan.cpp plan_pass), and verdicts and side data are scattered back to batch rows on the host.
constexpr uint64_t kSplitMinRows = 1ull << 18;

// The light region's row count and the device-row order (perm[d] = batch row), or 0 when the batch
// stays in order: the heavy rows must be between 1 % and 50 % of the rows and hold at least 30 % of
// the containers, in a batch of at least kSplitMinRows rows. KW_SPLIT=0 never splits, KW_SPLIT=1
// splits whenever both regions are non-empty (tests).
uint64_t split_rows(const Batch& B, std::vector<uint64_t>* perm) {
  const int mode = Knobs::num<KW_SPLIT>();
  if (mode == 0 || B.n == 0) return 0;
  const uint32_t thr = (uint32_t)Knobs::num<KW_HEAVY_CTR>();  // A/B knob: the container count above which a request is heavy
  auto heavy = [&](uint64_t r) { return B.ctr_off[r + 1] - B.ctr_off[r] > thr; };
  uint64_t nh = 0, ch = 0;
  for (uint64_t r = 0; r < B.n; ++r)
    if (heavy(r)) ++nh, ch += B.ctr_off[r + 1] - B.ctr_off[r];
  if (nh == 0 || nh == B.n) return 0;
  if (mode != 1 && (B.n < kSplitMinRows || nh * 100 < B.n || nh * 2 > B.n || ch * 10 < 3ull * B.containers())) return 0;
  perm->resize(B.n);
  uint64_t l = 0, h = B.n - nh;
  for (uint64_t r = 0; r < B.n; ++r) (*perm)[heavy(r) ? h++ : l++] = r;
  return B.n - nh;
}

// Batch rows in `perm` order as a new batch (P's row d = B's row perm[d]). with_bytes false: the
// device string columns get their offsets only — the upload gathers their bytes straight into its
// staging (gather_column) — and the host-only string columns stay empty. *order: the entity maps.
constexpr uint64_t kGatherTask = 1 << 16;
size_t gather_tasks(uint64_t m) { return (size_t)((m + kGatherTask - 1) / kGatherTask); }

void permute_batch(const Batch& B, const std::vector<uint64_t>& perm, Batch* P, bool with_bytes, RowOrder* order) {
  const uint64_t n = B.n;
  RowOrder& o = *order;
  o.perm = &perm;
  // an entity level: the destination offsets per parent and the source entity of each destination one
  auto level = [&](const std::vector<uint32_t>& off, uint64_t np, auto parent, std::vector<uint32_t>* doff,
                   std::vector<uint32_t>* emap) {
    doff->resize(np + 1);
    (*doff)[0] = 0;
    for (uint64_t d = 0; d < np; ++d) {
      const uint64_t p = parent(d);
      (*doff)[d + 1] = (*doff)[d] + (off[p + 1] - off[p]);
    }
    emap->resize((*doff)[np]);
    HostWorkers::get().run(gather_tasks(np), [&](size_t q) {
      for (uint64_t d = q * kGatherTask, e = std::min<uint64_t>(np, (q + 1) * kGatherTask); d < e; ++d) {
        const uint32_t s0 = off[parent(d)];
        for (uint32_t k = 0, c = (*doff)[d + 1] - (*doff)[d]; k < c; ++k) (*emap)[(*doff)[d] + k] = s0 + k;
      }
    });
  };
  auto gather_str = [&](const StrCol& src, uint64_t ne, auto map, StrCol* dst) {
    dst->off.resize(ne + 1);
    dst->off[0] = 0;
    for (uint64_t e = 0; e < ne; ++e) {
      const uint64_t s = map(e);
      dst->off[e + 1] = dst->off[e] + (src.off[s + 1] - src.off[s]);
    }
    if (!with_bytes) return;
    dst->bytes.assign(dst->off[ne], 0);
    HostWorkers::get().run(gather_tasks(ne), [&](size_t q) {
      for (uint64_t e = q * kGatherTask, f = std::min<uint64_t>(ne, (q + 1) * kGatherTask); e < f; ++e) {
        const uint64_t s = map(e);
        memcpy(dst->bytes.data() + dst->off[e], src.bytes.data() + src.off[s], src.off[s + 1] - src.off[s]);
      }
    });
  };
  P->n = n;
  auto row = [&](uint64_t d) { return perm[d]; };
  P->req_flags.resize(n);
  for (uint64_t d = 0; d < n; ++d) P->req_flags[d] = B.req_flags[perm[d]];
  gather_str(B.ns, n, row, &P->ns);
  if (with_bytes)
    for (auto [s, t] : {std::pair<const StrCol*, StrCol*>(&B.uid, &P->uid), std::pair<const StrCol*, StrCol*>(&B.op, &P->op),
                        std::pair<const StrCol*, StrCol*>(&B.kind, &P->kind), std::pair<const StrCol*, StrCol*>(&B.rkind, &P->rkind)})
      gather_str(*s, n, row, t);
  level(B.ctr_off, n, row, &P->ctr_off, &o.cmap);
  level(B.lbl_off, n, row, &P->lbl_off, &o.lmap);
  const uint64_t nc = o.cmap.size(), nl = o.lmap.size();
  auto ctr = [&](uint64_t e) { return (uint64_t)o.cmap[e]; };
  auto lbl = [&](uint64_t e) { return (uint64_t)o.lmap[e]; };
  P->ctr_flags.resize(nc);
  for (uint64_t e = 0; e < nc; ++e) P->ctr_flags[e] = B.ctr_flags[o.cmap[e]];
  gather_str(B.ctr_image, nc, ctr, &P->ctr_image);
  gather_str(B.ctr_aa, nc, ctr, &P->ctr_aa);
  if (with_bytes) gather_str(B.ctr_name, nc, ctr, &P->ctr_name);
  level(B.capadd_off, nc, ctr, &P->capadd_off, &o.amap);
  level(B.capdrop_off, nc, ctr, &P->capdrop_off, &o.dmap);
  gather_str(B.cap_add, o.amap.size(), [&](uint64_t e) { return (uint64_t)o.amap[e]; }, &P->cap_add);
  gather_str(B.cap_drop, o.dmap.size(), [&](uint64_t e) { return (uint64_t)o.dmap[e]; }, &P->cap_drop);
  gather_str(B.lbl_key, nl, lbl, &P->lbl_key);
  gather_str(B.lbl_val, nl, lbl, &P->lbl_val);
  if (with_bytes) P->finalize();
}

// String column m of the reordered batch P into `dst` (a piece of `bytes` bytes of the upload
// staging): every string from B by the entity maps, then the zero tail.
void gather_column(const Batch& B, const Batch& P, const RowOrder& o, int m, uint8_t* dst, size_t bytes) {
  const StrCol &s = host_str(B, m), &d = host_str(P, m);
  const uint64_t ne = d.n();
  HostWorkers::get().run(gather_tasks(ne), [&](size_t q) {
    for (uint64_t e = q * kGatherTask, f = std::min<uint64_t>(ne, (q + 1) * kGatherTask); e < f; ++e) {
      const uint64_t x = o.src(m, e);
      memcpy(dst + d.off[e], s.bytes.data() + s.off[x], s.off[x + 1] - s.off[x]);
    }
  });
  if (bytes > d.off[ne]) memset(dst + d.off[ne], 0, bytes - d.off[ne]);
}

int layout_batch(kw_batch* kb, int device, hipStream_t stream, std::vector<Piece>* pieces, bool may_split = false,
                 bool staging = true) {
  if (!kb || device < 0) return KW_E_ARG;
  HIPCHK(hipSetDevice(device));
  if (kb->dev) kb->dev.reset();  // re-upload: the previous device copy returns to the pools
  auto D = std::make_unique<DeviceBatch>();
  D->device = device;
  if (stream) {
    D->stream = stream;
    D->owns_stream = false;
  } else {
    HIPCHK(stream_pool().get(device, &D->stream));
  }
  kb->b.finalize();
  if (may_split) {
    D->split = split_rows(kb->b, &D->perm);
    if (D->split) {
      D->dev_b = std::make_unique<Batch>();
      D->order = std::make_unique<RowOrder>();
      permute_batch(kb->b, D->perm, D->dev_b.get(), /*with_bytes=*/false, D->order.get());
    } else {
      D->perm.clear();
    }
  }
  const Batch& B = D->dev_b ? *D->dev_b : kb->b;
  pieces->clear();
  size_t total = 0;
  auto add = [&](const void* src, size_t bytes, PieceKind k, int m) {
    size_t at = total;
    pieces->push_back({src, bytes, at, k, m, false});
    total += (bytes + 255) & ~(size_t)255;
    return at;
  };
  size_t o_rf = add(B.req_flags.data(), B.req_flags.size(), PK_ROW_U8, -1);
  size_t o_co = add(B.ctr_off.data(), B.ctr_off.size() * 4, PK_ROW_OFF, -1);
  size_t o_lo = add(B.lbl_off.data(), B.lbl_off.size() * 4, PK_ROW_OFF, -1);
  size_t o_cf = add(B.ctr_flags.data(), B.ctr_flags.size(), PK_CTR_U8, -1);
  size_t o_ca = add(B.capadd_off.data(), B.capadd_off.size() * 4, PK_CTR_OFF, -1);
  size_t o_cd = add(B.capdrop_off.data(), B.capdrop_off.size() * 4, PK_CTR_OFF, -1);
  size_t c_off[NSTR], c_bytes[NSTR];
  for (int m = 0; m < (int)NSTR; ++m) {
    const StrCol& c = host_str(B, m);
    c_off[m] = add(c.off.data(), c.off.size() * 4, PK_STR_OFF, m);
    if (D->order) {  // reordered: gathered into the staging at upload (>= 16 B zero tail, StrCol::pad)
      c_bytes[m] = add(nullptr, ((size_t)c.off.back() + 31) & ~(size_t)15, PK_STR_BYTES, m);
      pieces->back().gather = true;
    } else {
      c_bytes[m] = add(c.bytes.data(), c.bytes.size(), PK_STR_BYTES, m);
    }
  }
  total = std::max<size_t>(total, 256);
  void* dcols = nullptr;
  HIPCHK(dev_pool().alloc(device, total, &dcols));
  D->cols = (uint8_t*)dcols;
  D->cols_bytes = total;
  if (staging) {
    HIPCHK(host_pool().alloc(device, total, &D->staging));
    D->staging_bytes = total;
  }
  D->cur = D->stream;
  D->req_flags = D->cols + o_rf;
  D->ctr_off = (const uint32_t*)(D->cols + o_co);
  D->lbl_off = (const uint32_t*)(D->cols + o_lo);
  D->ctr_flags = D->cols + o_cf;
  D->capadd_off = (const uint32_t*)(D->cols + o_ca);
  D->capdrop_off = (const uint32_t*)(D->cols + o_cd);
  for (int m = 0; m < (int)NSTR; ++m) {
    const StrCol& c = host_str(B, m);
    DeviceBatch::DCol& d = D->str[m];
    d.off = (const uint32_t*)(D->cols + c_off[m]);
    d.bytes = D->cols + c_bytes[m];
    d.n = c.n();
    d.nbytes = c.off.back();
  }
  kb->dev = std::move(D);
  return KW_OK;
}

int upload_batch(kw_batch* kb, int device, hipStream_t stream, bool sync) {
  std::vector<Piece> pieces;
  if (int rc = layout_batch(kb, device, stream, &pieces, /*may_split=*/true)) return rc;
  DeviceBatch& D = *kb->dev;
  uint8_t* st = (uint8_t*)D.staging;
  for (auto& p : pieces) {
    if (!p.bytes) continue;
    if (p.gather)
      gather_column(kb->b, *D.dev_b, *D.order, p.m, st + p.at, p.bytes);
    else
      parallel_copy(st + p.at, p.src, p.bytes);
  }
  D.order.reset();  // (the planner reads the reordered batch's offsets only)
  HIPCHK(hipMemcpyAsync(D.cols, st, D.cols_bytes, hipMemcpyHostToDevice, D.stream));
  if (sync) HIPCHK(hipStreamSynchronize(D.stream));
  D.loaded = ~0u;
  return KW_OK;
}

// Byte range [lo, hi) of piece p that rows [r0, r1) occupy. A chunk's string bytes run 64 bytes past
// its last string (the device's batched reads past a string end stay inside uploaded bytes); the
// first chunk starts at 0 and the last runs to the piece's end (its zero padding).
void piece_range(const Batch& B, const Piece& p, uint64_t r0, uint64_t r1, bool last, size_t* lo, size_t* hi) {
  size_t a = 0, e = 0;
  uint64_t g0 = 0, g1 = 0;
  switch (p.kind) {
    case PK_ROW_U8: a = r0; e = r1; break;
    case PK_ROW_OFF: a = 4 * r0; e = 4 * (r1 + 1); break;
    case PK_CTR_U8: a = B.ctr_off[r0]; e = B.ctr_off[r1]; break;
    case PK_CTR_OFF: a = 4ull * B.ctr_off[r0]; e = 4ull * ((uint64_t)B.ctr_off[r1] + 1); break;
    case PK_STR_OFF: str_range(B, p.m, r0, r1, &g0, &g1); a = 4 * g0; e = 4 * (g1 + 1); break;
    case PK_STR_BYTES: {
      str_range(B, p.m, r0, r1, &g0, &g1);
      const StrCol& c = host_str(B, p.m);
      a = c.off[g0];
      e = (size_t)c.off[g1] + 64;
      break;
    }
  }
  if (r0 == 0) a = 0;
  if (last) e = p.bytes;
  *lo = std::min(a, p.bytes);
  *hi = std::min(std::max(e, a), p.bytes);
}

// The pass's side data into the batch's host copy (kw_batch_wide_arg, the formatter): entity
// indices >= 65535 and > 15-member group causes (kernels.hpp WideRec), after the pass on stream s.
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

// Bulk host -> host validation (kw_validate_host): the batch's columns are uploaded, evaluated and
// read back in row chunks whose stages overlap: the host workers build chunk k's tile descriptors
// and fill its pinned staging while the copy engines move chunk k-1 in and chunk k-2's verdicts out
// and the tile kernel evaluates in between (three streams ordered by events). Only the string
// columns the pass reads are uploaded. The plan's tile capacities come from a sample of the tile
// needs (every stride-th tile), and each chunk's descriptors are built just before its fill, so the
// first read-back starts after one small chunk rather than after a whole-batch head; a request
// that exceeds the capacities alone runs through the overflow kernels right after its chunk's tile
// launch. Passes with several launches, wide side data or NFA elements run unchunked (upload, pass,
// read-back) with the same result.
int validate_host(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, int device,
                  uint32_t* out, size_t count, uint32_t chunk_rows) {
  if (!env || !kb || !out || !policies || npol == 0) return KW_E_ARG;
  if (env->e.device < 0 || !env->e.d_blob) return KW_E_DEVICE;
  if (device != env->e.device || count != kb->b.n * (uint64_t)npol) return KW_E_ARG;
  // diagnostics (KW_BULK_DEBUG=1): host wall time of each stage, printed at the end
  const bool dbg = Knobs::on<KW_BULK_DEBUG>();
  using clk = std::chrono::steady_clock;
  const auto t_start = clk::now();
  double t_layout = 0, t_plan = 0, t_prep = 0, t_desc = 0, t_fill = 0, t_enq = 0, t_out = 0, t_first = -1;
  auto since = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
  std::vector<Piece> pieces;
  if (int rc = layout_batch(kb, device, nullptr, &pieces, /*may_split=*/false, /*staging=*/false)) return rc;
  t_layout = since(t_start);
  DeviceBatch& D = *kb->dev;
  const Batch& B = kb->b;
  D.loaded = ~0u;  // (planned as if resident; set to the pass's columns below)
  // tile capacities from about 2048 sampled tiles (KW_BULK_SAMPLE=0: every tile, A/B knob)
  const bool sample = Knobs::on<KW_BULK_SAMPLE>();
  D.needs_stride = sample ? (uint32_t)std::max<uint64_t>(1, B.n / ((uint64_t)kSlotRows * 2048)) : 1u;
  PassPlan plan;
  const int prc = validate_common(env, kb, policies, npol, nullptr, origin, &plan);
  D.needs_stride = 1;
  if (prc) {
    D.loaded = 0;
    return prc;
  }
  const uint32_t need = plan.geom.need;
  t_plan = since(t_start) - t_layout;
  auto wanted = [&](const Piece& p) { return p.m < 0 || ((need >> p.m) & 1u); };
  // columns page-locked in place (kw_batch_pin_host) go to the device by DMA from where they lie;
  // the others through the pinned staging, filled by the host workers
  std::vector<char> dma(pieces.size(), 0);
  if (!kb->host_pinned.empty())
    for (size_t i = 0; i < pieces.size(); ++i) {
      hipPointerAttribute_t pa;
      dma[i] = pieces[i].bytes && hipPointerGetAttributes(&pa, pieces[i].src) == hipSuccess &&
               pa.type == hipMemoryTypeHost;
      (void)hipGetLastError();
    }
  hipStream_t sc = D.stream;
  EvalArgs A;
  // (NFA elements: their pre-pass reads whole columns, so such passes are not chunked)
  const bool chunked = plan.tiles.size() == 1 && plan.wide.groups.empty() && plan.nwide == 0 && !plan.rows_mode &&
                       !(plan.geom.debug & 512u) && !(plan.geom.feat & kFeatNfa) && B.n > 0;
  // the staging image of the whole batch only where it is used: the unchunked path and per-range
  // copies (packed chunks go through their own ring; pinning C5's 3.6 GB image cost 360 ms a call)
  const bool pack_knob = Knobs::on<KW_BULK_PACK>();
  if ((!chunked || !pack_knob) && !D.staging) {
    HIPCHK(host_pool().alloc(device, D.cols_bytes, &D.staging));
    D.staging_bytes = D.cols_bytes;
  }
  uint8_t* st = (uint8_t*)D.staging;
  if (!chunked) {  // one upload, the full pass, one read-back
    std::vector<CopySeg> segs;
    for (size_t i = 0; i < pieces.size(); ++i)
      if (pieces[i].bytes && !dma[i]) segs.push_back({st + pieces[i].at, pieces[i].src, pieces[i].bytes});
    parallel_copy_segs(segs);
    for (const CopySeg& c : segs)
      HIPCHK(hipMemcpyAsync(D.cols + ((uint8_t*)c.dst - st), c.dst, c.bytes, hipMemcpyHostToDevice, sc));
    for (size_t i = 0; i < pieces.size(); ++i)
      if (pieces[i].bytes && dma[i])
        HIPCHK(hipMemcpyAsync(D.cols + pieces[i].at, pieces[i].src, pieces[i].bytes, hipMemcpyHostToDevice, sc));
    if (int rc = run_validate(env, kb, plan, origin, false, sc)) return rc;
    return kw_batch_verdicts(kb, out, count);
  }
  D.last_big_stride = 0;  // (no wide groups in a chunked pass: stale cause bitsets must not be read)
  D.last_big_ref.clear();
  if (int rc = prepare_pass(kb, plan, sc, &A, /*descs=*/false)) {
    D.loaded = 0;
    return rc;
  }
  t_prep = since(t_start) - t_layout - t_plan;
  D.loaded = need;
  const TileArgs& G = plan.geom;
  const uint64_t ntiles = (B.n + G.rows - 1) / G.rows;
  const uint64_t def_chunk = (uint64_t)Knobs::num<KW_BULK_CHUNK>();  // A/B knob (profiles/r04_bulk_sweep.txt)
  const uint64_t per = chunk_rows ? chunk_rows : def_chunk;
  // chunk k: tiles [tb[k], tb[k+1]). The read-back stream is the longest (4 B x npol per request
  // out vs the request's columns in), so the first chunks are small (1/16 of `per`, doubling) to
  // start it early; then `per` rows a chunk.
  const bool ramp = Knobs::on<KW_BULK_RAMP>();  // A/B knob
  // The last chunks shrink the same way (r05): the final chunk's read-back overlaps nothing, so a
  // full-size last chunk left ~1 ms of C4's read-back exposed. At most ~240 chunks (per grows).
  const uint64_t tper = std::max<uint64_t>({1, per / G.rows, (ntiles + 239) / 240});
  std::vector<uint64_t> tb{0};
  {
    std::vector<uint64_t> head, tail;  // chunk sizes in tiles, from the front and from the back
    uint64_t left = ntiles, sh = ramp ? std::max<uint64_t>(1, tper / 16) : tper, st_ = sh;
    while (left) {
      head.push_back(std::min(sh, left));
      left -= head.back();
      sh = std::min(tper, sh * 2);
      if (!left || !ramp) continue;
      tail.push_back(std::min(st_, left));
      left -= tail.back();
      st_ = std::min(tper, st_ * 2);
    }
    for (uint64_t h : head) tb.push_back(tb.back() + h);
    for (auto it = tail.rbegin(); it != tail.rend(); ++it) tb.push_back(tb.back() + *it);
  }
  const uint64_t K = tb.size() - 1;
  auto row_of = [&](uint64_t t) { return std::min<uint64_t>(B.n, t * G.rows); };
  hipPointerAttribute_t attr;
  const bool direct = Knobs::on<KW_BULK_DIRECT>();  // A/B knob
  const bool pinned = direct && hipPointerGetAttributes(&attr, out) == hipSuccess && attr.type == hipMemoryTypeHost;
  (void)hipGetLastError();  // a pageable pointer leaves an error state behind
  // pinned output: at most `depth` chunks in flight past the read-back. Unbounded, the host queues
  // every chunk's copies and launch at once and the copies run slower (C4 1M: 16.0-16.7 ms vs
  // 9.7-10.9 at depth 2, profiles/r04_bulk_modes.txt). Staged columns take 3 (the host fills pace
  // the uploads), columns DMA'd in place 2 (at 3 their uploads crowd the read-backs: 11.0 vs
  // 7.1 ms, profiles/r04_bulk_sweep.txt). KW_BULK_DEPTH: A/B knob, 0 = unbounded.
  const int depth_knob = Knobs::num<KW_BULK_DEPTH>();
  const bool any_dma = std::count(dma.begin(), dma.end(), 1) > 0;
  const uint64_t depth = depth_knob >= 0 ? (uint64_t)depth_knob : (any_dma ? 2 : 3);
  // (the largest chunk: `per` grows past ~240 chunks)
  uint64_t max_rows = 0;
  for (uint64_t k = 0; k < K; ++k) max_rows = std::max(max_rows, row_of(tb[k + 1]) - row_of(tb[k]));
  const size_t bounce_bytes = (size_t)max_rows * npol * 4;
  void* bounce[2] = {nullptr, nullptr};
  // descriptors: two halves of `dcap` on the device and in pinned host memory (chunk k uses half
  // k & 1; half reuse waits for chunk k-2's kernel on the device and its upload on the host)
  uint64_t dcap = tper + tper / 4 + 64;
  void* hdesc = nullptr;
  size_t hdesc_bytes = 0;
  hipStream_t s_in = nullptr, s_out = nullptr;
  std::vector<hipEvent_t> ev(3 * K, nullptr);
  int rc = KW_OK;  // (a failure below leaves the batch's columns partly uploaded: D.loaded is cleared)
  auto fail = [&](hipError_t e) {
    if (e != hipSuccess && rc == KW_OK) rc = KW_E_DEVICE;
    return e != hipSuccess;
  };
  auto code = [&](int c) {
    if (c != KW_OK && rc == KW_OK) rc = c;
    return c != KW_OK;
  };
  if (!pinned)
    for (auto& b : bounce)
      if (fail(host_pool().alloc(device, bounce_bytes, &b))) break;
  auto alloc_descs = [&]() {
    if (hdesc) host_pool().release(device, hdesc, hdesc_bytes);
    hdesc = nullptr;
    hdesc_bytes = (size_t)(2 * dcap) * sizeof(TileDesc);
    if (fail(host_pool().alloc(device, hdesc_bytes, &hdesc))) return false;
    return !code(ensure(&D.desc, &D.desc_cap, (size_t)(2 * dcap)));
  };
  if (rc == KW_OK) (void)alloc_descs();
  // staged columns: each chunk's ranges packed into one pinned slot, one H2D into the device slot,
  // then the scatter kernel puts them in place (one copy per chunk, not one per column). kRing
  // slots: packing chunk k waits for chunk k - kRing's upload. KW_BULK_PACK=0: a copy per column
  // range (A/B knob, profiles/r05_bulk_copies.txt).
  constexpr uint64_t kRing = 4;
  // (the scatter kernel's argument holds kMaxScatterSegs ranges: a layout with more staged pieces
  // than that — none today, 6 row pieces + 2 per string column — copies each range on its own)
  const bool packed = pack_knob && std::count(dma.begin(), dma.end(), 0) > 0 &&
                      (size_t)std::count(dma.begin(), dma.end(), 0) <= kMaxScatterSegs;
  size_t slot_bytes = 0;
  void *hpack = nullptr, *dland = nullptr;
  if (packed && rc == KW_OK) {
    for (uint64_t k = 0; k < K; ++k) {
      size_t b = 0;
      for (size_t i = 0; i < pieces.size(); ++i) {
        if (!wanted(pieces[i]) || dma[i]) continue;
        size_t lo, hi;
        piece_range(B, pieces[i], row_of(tb[k]), row_of(tb[k + 1]), k + 1 == K, &lo, &hi);
        if (hi > lo) b += (hi - lo) + 32;
      }
      slot_bytes = std::max(slot_bytes, (b + 255) & ~(size_t)255);
    }
    if (!fail(host_pool().alloc(device, kRing * slot_bytes, &hpack))) (void)fail(dev_pool().alloc(device, kRing * slot_bytes, &dland));
  }
  StreamPool& SP = stream_pool();
  if (rc == KW_OK && !fail(SP.get(device, &s_in)) && !fail(SP.get(device, &s_out)))
    for (auto& e : ev)
      if (fail(SP.get(device, &e))) break;
  auto copy_out = [&](uint64_t k) {
    const auto t0 = clk::now();
    if (pinned || rc != KW_OK || fail(hipEventSynchronize(ev[3 * k + 2]))) return;
    const uint64_t r0 = row_of(tb[k]), r1 = row_of(tb[k + 1]);
    parallel_copy_segs({{out + r0 * npol, bounce[k & 1], (size_t)(r1 - r0) * npol * 4}});
    t_out += since(t0);
  };
  // overflow requests (alone beyond the tile capacities): their list, classes and side data
  uint64_t n_ovf = 0;
  std::vector<TileDesc> cd;
  std::vector<uint32_t> co;
  for (uint64_t k = 0; k < K && rc == KW_OK; ++k) {
    const uint64_t r0 = row_of(tb[k]), r1 = row_of(tb[k + 1]);
    if (pinned && depth && k >= depth && fail(hipEventSynchronize(ev[3 * (k - depth) + 2]))) break;
    // the chunk's columns first: their H2D starts at once, and the descriptor build below then
    // reads offsets the fill has just brought into the host caches
    std::vector<CopySeg> segs, dsegs;  // (staged, direct)
    const size_t slot = (size_t)(k % kRing) * slot_bytes;
    ScatterArgs sa;
    sa.dst = D.cols;
    sa.src = (const uint8_t*)dland + slot;
    sa.nseg = 0;
    size_t pk = 0;  // packed bytes of the chunk (each range at its device offset's residue mod 16)
    for (size_t i = 0; i < pieces.size(); ++i) {
      const Piece& p = pieces[i];
      if (!wanted(p)) continue;
      size_t lo, hi;
      piece_range(B, p, r0, r1, k + 1 == K, &lo, &hi);
      if (hi <= lo) continue;
      if (dma[i]) {
        dsegs.push_back({D.cols + p.at + lo, (const uint8_t*)p.src + lo, hi - lo});
      } else if (packed) {
        const size_t at = ((pk + 15) & ~(size_t)15) + ((p.at + lo) & 15);
        segs.push_back({(uint8_t*)hpack + slot + at, (const uint8_t*)p.src + lo, hi - lo});
        sa.seg[sa.nseg++] = {p.at + lo, at, hi - lo};
        pk = at + (hi - lo);
      } else {
        segs.push_back({st + p.at + lo, (const uint8_t*)p.src + lo, hi - lo});
      }
    }
    if (packed && k >= kRing && fail(hipEventSynchronize(ev[3 * (k - kRing)]))) break;  // its slot's upload is done
    const auto t0 = clk::now();
    parallel_copy_segs(segs);
    t_fill += since(t0);
    const auto t1 = clk::now();
    for (const CopySeg& c : dsegs)
      if (fail(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyHostToDevice, s_in))) break;
    if (packed) {
      if (pk && (fail(hipMemcpyAsync((uint8_t*)dland + slot, (uint8_t*)hpack + slot, pk, hipMemcpyHostToDevice, s_in)) ||
                 fail(launch_scatter(sa, s_in))))
        break;
    } else {
      for (const CopySeg& c : segs)
        if (rc != KW_OK ||
            fail(hipMemcpyAsync(D.cols + ((uint8_t*)c.dst - st), c.dst, c.bytes, hipMemcpyHostToDevice, s_in)))
          break;
    }
    if (rc != KW_OK) break;
    t_enq += since(t1);
    const auto td = clk::now();
    cd.clear();
    co.assign(1, 0u);
    if (code(build_descs(B, G, 0, B.n, tb[k], tb[k + 1], 128, &cd, &co))) break;
    co[0] = (uint32_t)(co.size() - 1);
    if (cd.size() > dcap) {  // more split tiles than the halves hold: wait for every launch, regrow
      if (fail(hipStreamSynchronize(s_in)) || fail(hipStreamSynchronize(sc))) break;
      dcap = cd.size() + cd.size() / 4 + 64;
      if (!alloc_descs()) break;
    } else if (k >= 2 && fail(hipEventSynchronize(ev[3 * (k - 2)]))) {  // host half free: its upload is done
      break;
    }
    TileDesc* hd = (TileDesc*)hdesc + (k & 1) * dcap;
    if (!cd.empty()) memcpy(hd, cd.data(), cd.size() * sizeof(TileDesc));
    t_desc += since(td);
    const auto t2 = clk::now();
    TileDesc* dd = D.desc + (k & 1) * dcap;
    if (k >= 2 && fail(hipStreamWaitEvent(s_in, ev[3 * (k - 2) + 1], 0))) break;  // device half free
    if (!cd.empty() && fail(hipMemcpyAsync(dd, hd, cd.size() * sizeof(TileDesc), hipMemcpyHostToDevice, s_in))) break;
    if (fail(hipEventRecord(ev[3 * k], s_in)) || fail(hipStreamWaitEvent(sc, ev[3 * k], 0))) break;
    EvalArgs Ak = A;
    Ak.ndesc = cd.size();
    if (!sched_dynamic(cd.size(), plan.grid, plan.geom.lds_tables != 0)) Ak.sched = nullptr;
    if (!cd.empty() && fail(launch_evaluate_tiles(Ak, plan.tiles[0], D.d_tiles, dd, plan.grid, sc))) break;
    if (co[0]) {  // rare: synchronous set-up, then the overflow kernels on the chunk's requests
      if (fail(hipStreamSynchronize(sc))) break;
      if (n_ovf == 0 && fail(hipMemsetAsync(D.wide_count, 0, sizeof(uint32_t), sc))) break;  // (first overflow chunk)
      D.wide_valid = true;
      n_ovf += co[0];
      if (code(ensure(&D.overflow, &D.overflow_cap, co.size())) || code(ensure_overflow_classes(B, &D, G, &A))) break;
      const size_t cap = (size_t)n_ovf * plan.wide_cap_per_row;
      if (cap > D.wide_rec_cap || !D.wide_rec) {  // grow, keeping the records earlier chunks wrote
        WideRec* old = D.wide_rec;
        const size_t old_cap = D.wide_rec_cap;
        D.wide_rec = nullptr;
        D.wide_rec_cap = 0;
        if (code(ensure(&D.wide_rec, &D.wide_rec_cap, std::max(cap, 2 * old_cap)))) break;
        if (old && fail(hipMemcpy(D.wide_rec, old, old_cap * sizeof(WideRec), hipMemcpyDeviceToDevice))) break;
        if (old) dev_pool().release(device, old, old_cap * sizeof(WideRec));
      }
      A.wide_rec = D.wide_rec;
      A.wide_cap = (uint32_t)std::min<size_t>(D.wide_rec_cap, 0xffffffffu);
      Ak = A;
      if (fail(hipMemcpy(D.overflow, co.data(), co.size() * sizeof(uint32_t), hipMemcpyHostToDevice))) break;
      if (fail(launch_overflow(Ak, D.d_tiles, D.overflow, co[0], sc))) break;
    }
    if (fail(hipEventRecord(ev[3 * k + 1], sc)) || fail(hipStreamWaitEvent(s_out, ev[3 * k + 1], 0))) break;
    uint32_t* dst = pinned ? out + r0 * npol : (uint32_t*)bounce[k & 1];
    if (fail(hipMemcpyAsync(dst, D.verdicts + r0 * npol, (size_t)(r1 - r0) * npol * 4, hipMemcpyDeviceToHost, s_out))) break;
    if (fail(hipEventRecord(ev[3 * k + 2], s_out))) break;
    t_enq += since(t2);
    if (k == 0) t_first = since(t_start);
    if (k >= 1) copy_out(k - 1);  // (bounce[k & 1] was last read by chunk k - 2's copy-out)
  }
  if (rc == KW_OK) copy_out(K - 1);
  const auto t_w = clk::now();
  if (s_in) (void)hipStreamSynchronize(s_in);
  (void)hipStreamSynchronize(sc);
  if (s_out) (void)hipStreamSynchronize(s_out);
  const double t_wait = since(t_w);
  const auto t_td = clk::now();
  for (auto& e : ev) SP.put(device, e);
  SP.put(device, s_in);
  SP.put(device, s_out);
  for (auto& b : bounce) host_pool().release(device, b, bounce_bytes);
  if (hdesc) host_pool().release(device, hdesc, hdesc_bytes);
  if (hpack) host_pool().release(device, hpack, kRing * slot_bytes);
  if (dland) dev_pool().release(device, dland, kRing * slot_bytes);
  D.last_wide_cap = A.wide_cap;
  D.cur = sc;
  if (rc != KW_OK) {
    D.loaded = 0;
    return rc;
  }
  rc = load_side_data(kb, sc);  // overflow requests' wide arguments (kw_batch_wide_arg)
  if (dbg)
    fprintf(stderr,
            "[kw bulk] rows %llu chunks %llu pinned %d direct-columns %d overflow %llu: layout %.2f plan %.2f prepare %.2f "
            "descs %.2f fill %.2f enqueue %.2f copy-out %.2f first chunk queued at %.2f, final wait %.2f, teardown %.2f, "
            "total %.2f ms\n",
            (unsigned long long)B.n, (unsigned long long)K, pinned ? 1 : 0, (int)std::count(dma.begin(), dma.end(), 1),
            (unsigned long long)n_ovf, t_layout, t_plan, t_prep, t_desc, t_fill, t_enq, t_out, t_first, t_wait, since(t_td),
            since(t_start));
  return rc;
}
}  // namespace

extern "C" {

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

int kw_batch_pin_host(kw_batch* kb, int device) {
  if (!kb || device < 0) return KW_E_ARG;
  if (!kb->host_pinned.empty()) return KW_OK;
  HIPCHK(hipSetDevice(device));
  Batch& B = kb->b;
  B.finalize();  // (pads the byte pools now: later passes do not resize what is registered)
  std::vector<std::pair<void*, size_t>> cols = {
      {B.req_flags.data(), B.req_flags.size()},   {B.ctr_off.data(), B.ctr_off.size() * 4},
      {B.lbl_off.data(), B.lbl_off.size() * 4},   {B.ctr_flags.data(), B.ctr_flags.size()},
      {B.capadd_off.data(), B.capadd_off.size() * 4}, {B.capdrop_off.data(), B.capdrop_off.size() * 4}};
  for (int m = 0; m < (int)NSTR; ++m) {
    const StrCol& c = host_str(B, m);
    cols.push_back({(void*)c.off.data(), c.off.size() * 4});
    cols.push_back({(void*)c.bytes.data(), c.bytes.size()});
  }
  // small arrays may share a page with another allocation: they stay pageable (staged), as does
  // any array the runtime declines to register
  for (const auto& [p, n] : cols) {
    if (n < ((size_t)1 << 16)) continue;
    if (hipHostRegister(p, n, hipHostRegisterDefault) == hipSuccess)
      kb->host_pinned.push_back(p);
    else
      (void)hipGetLastError();
  }
  return KW_OK;
}

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

int kw_batch_verdicts(kw_batch* b, uint32_t* host_out, size_t count) {
  if (!b || !b->dev || (!host_out && count)) return KW_E_ARG;
  DeviceBatch& D = *b->dev;
  if (count > D.last_verdicts) return KW_E_ARG;
  HIPCHK(hipSetDevice(D.device));
  hipStream_t s = D.cur ? D.cur : D.stream;
  const size_t vbytes = count * sizeof(uint32_t);
  constexpr size_t kBounce = (size_t)64 << 20;
  if (D.split && count) {
    // rows in device order (light / heavy split): whole device rows through a pinned bounce block,
    // each scattered to its batch row's words below `count`
    const uint64_t rw = std::max<uint32_t>(D.last_row_words, 1), nrows = D.last_verdicts / rw;
    const uint64_t per = std::max<uint64_t>(1, kBounce / (rw * 4));
    void* bounce = nullptr;
    HIPCHK(host_pool().alloc(D.device, kBounce, &bounce));
    for (uint64_t d0 = 0; d0 < nrows; d0 += per) {
      const uint64_t d1 = std::min(nrows, d0 + per);
      HIPCHK(hipMemcpyAsync(bounce, D.verdicts + d0 * rw, (d1 - d0) * rw * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      const uint32_t* src = (const uint32_t*)bounce;
      HostWorkers::get().run((size_t)((d1 - d0 + 4095) / 4096), [&](size_t q) {
        for (uint64_t d = d0 + q * 4096, e = std::min(d1, d0 + (q + 1) * 4096); d < e; ++d) {
          const uint64_t w0 = D.perm[d] * rw;
          if (w0 < count) memcpy(host_out + w0, src + (d - d0) * rw, std::min<uint64_t>(rw, count - w0) * 4);
        }
      });
    }
    host_pool().release(D.device, bounce, kBounce);
  } else if (vbytes > ((size_t)16 << 20)) {
    // large read-backs through a pinned bounce block (full-rate DMA), fanned out to the caller's
    // (pageable) buffer by several threads
    void* bounce = nullptr;
    HIPCHK(host_pool().alloc(D.device, kBounce, &bounce));
    for (size_t at = 0; at < vbytes; at += kBounce) {
      const size_t n = std::min(kBounce, vbytes - at);
      HIPCHK(hipMemcpyAsync(bounce, (const uint8_t*)D.verdicts + at, n, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      parallel_copy((uint8_t*)host_out + at, bounce, n);
    }
    host_pool().release(D.device, bounce, kBounce);
  } else if (count) {
    HIPCHK(hipMemcpyAsync(host_out, D.verdicts, vbytes, hipMemcpyDeviceToHost, s));
  }
  return load_side_data(b, s);
}

int kw_debug_plan(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, uint32_t* out,
                  int cap) {
  if (!env || !kb || !out || cap < 8 || (!policies && npol)) return KW_E_ARG;
  // plan against a host view of the batch (no device memory, nothing launched), in the device-row
  // order kw_batch_to_device would give it
  std::unique_ptr<DeviceBatch> saved = std::move(kb->dev);
  kb->b.finalize();
  std::vector<uint64_t> perm;
  const uint64_t split = split_rows(kb->b, &perm);
  std::unique_ptr<Batch> P;
  if (split) {
    P = std::make_unique<Batch>();
    RowOrder o;
    permute_batch(kb->b, perm, P.get(), /*with_bytes=*/false, &o);
  }
  const Batch& B = P ? *P : kb->b;
  auto D = std::make_unique<DeviceBatch>();
  D->split = split;
  D->perm = std::move(perm);
  static uint32_t dummy;
  D->req_flags = B.req_flags.data();
  D->ctr_off = B.ctr_off.data();
  D->lbl_off = B.lbl_off.data();
  D->ctr_flags = B.ctr_flags.data();
  D->capadd_off = B.capadd_off.data();
  D->capdrop_off = B.capdrop_off.data();
  for (int m = 0; m < (int)NSTR; ++m) {
    const StrCol& c = host_str(B, m);
    D->str[m] = {c.off.data(), c.bytes.empty() ? (const uint8_t*)&dummy : c.bytes.data(), c.n(), c.off.back()};
  }
  D->verdicts = &dummy;
  D->dev_b = std::move(P);
  kb->dev = std::move(D);
  PassPlan plan;
  int rc = plan_pass(env, kb, policies, npol, nullptr, origin, Knobs::on<KW_BULK_DEBUG>(), &plan);
  const TileArgs& T = plan.geom;
  const uint32_t vals[8] = {T.lds_bytes, (uint32_t)plan.launches.size(), (uint32_t)plan.chunks.size(), T.lds_tables,
                            T.rows, T.cmax, T.kmax, T.lmax};
  for (int i = 0; i < 8; ++i) out[i] = rc == KW_OK ? vals[i] : 0u;
  if (cap >= 16) {  // regions: count, light rows, the first region's grid, the heavy region's LDS / rows / cmax / grid, scan regions
    const bool two = rc == KW_OK && plan.regions.size() == 2;
    const TileArgs* H = two ? &plan.regions[1].geom : nullptr;
    uint32_t more[8] = {rc == KW_OK ? (uint32_t)plan.regions.size() : 0u, (uint32_t)split,
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

int kw_validate_timed(const kw_env* env, kw_batch* b, const int32_t* policies, uint32_t npol, int origin, int warmup,
                      int reps, kw_timing* out) {
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

int kw_metrics_render(const kw_metrics* m, char* buf, size_t cap, size_t* need) {
  if (!m) return KW_E_ARG;
  return put_out(m->m.render(), buf, cap, need);
}

void kw_metrics_reset(kw_metrics* m) {
  if (m) m->m.reset();
}
