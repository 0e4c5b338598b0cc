// upload.cpp — the host batch to the device image (upload.hpp): row split, layout, whole-batch
// upload, page-locking of the host columns and the planner's host view.
#include "upload.hpp"

#include <algorithm>
#include <cstring>

#include "knobs.hpp"
#include "pass.hpp"
#include "plan.hpp"

namespace kw {

// ---- light / heavy split at upload. A batch whose container counts
// are heavy-tailed (C5: Zipf over 1..64 — 14.7 % of the requests hold 63 % of the containers) sizes
// every tile's capacities, and so the occupancy, by the heavy requests scattered through it. The
// device copy instead holds the light requests (<= KW_HEAVY_CTR containers, 5) first and the heavy
// ones after them, in batch order within each region; the planner gives each region its own tile
// geometry (plan.cpp plan_pass), and verdicts and side data are scattered back to batch rows on the host.
constexpr uint64_t kSplitMinRows = 1ull << 18;

bool page_locked(const void* p) {
  hipPointerAttribute_t a;
  const bool host = p && hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost;
  (void)hipGetLastError();  // a pageable pointer leaves an error state behind
  return host;
}

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

constexpr uint64_t kGatherTask = 1 << 16;
static size_t gather_tasks(uint64_t m) { return (size_t)((m + kGatherTask - 1) / kGatherTask); }

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
static void gather_column(const Batch& B, const Batch& P, const RowOrder& o, int m, uint8_t* dst, size_t bytes) {
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

// Points D's column views at ptr[i], the i-th column of for_each_column(B).
static void set_views(DeviceBatch* D, const Batch& B, const std::vector<const uint8_t*>& ptr) {
  D->req_flags = ptr[0];
  D->ctr_off = (const uint32_t*)ptr[1];
  D->lbl_off = (const uint32_t*)ptr[2];
  D->ctr_flags = ptr[3];
  D->capadd_off = (const uint32_t*)ptr[4];
  D->capdrop_off = (const uint32_t*)ptr[5];
  for (int m = 0; m < (int)NSTR; ++m) {
    const StrCol& c = host_str(B, m);
    D->str[m] = {(const uint32_t*)ptr[6 + 2 * m], ptr[7 + 2 * m], c.n(), c.off.back()};
  }
}

int layout_batch(kw_batch* kb, int device, hipStream_t stream, std::vector<Piece>* pieces, bool may_split, bool staging) {
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
  for_each_column(B, [&](PieceKind k, int m, const void* src, size_t bytes) {
    // reordered: string bytes are gathered into the staging at upload (>= 16 B zero tail, StrCol::pad)
    const bool gather = k == PK_STR_BYTES && D->order;
    if (gather) bytes = ((size_t)host_str(B, m).off.back() + 31) & ~(size_t)15;
    pieces->push_back({gather ? nullptr : src, bytes, total, k, m, gather});
    total += (bytes + 255) & ~(size_t)255;
  });
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
  std::vector<const uint8_t*> ptr;
  for (const Piece& p : *pieces) ptr.push_back(D->cols + p.at);
  set_views(D.get(), B, ptr);
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

int pin_host(kw_batch* kb, int device) {
  if (!kb || device < 0) return KW_E_ARG;
  if (!kb->host_pinned.empty()) return KW_OK;
  HIPCHK(hipSetDevice(device));
  kb->b.finalize();  // (pads the byte pools now: later passes do not resize what is registered)
  // small arrays may share a page with another allocation: they stay pageable (staged), as does
  // any array the runtime declines to register
  for_each_column(kb->b, [&](PieceKind, int, const void* p, size_t n) {
    if (n < ((size_t)1 << 16)) return;
    if (hipHostRegister((void*)p, n, hipHostRegisterDefault) == hipSuccess)
      kb->host_pinned.push_back((void*)p);
    else
      (void)hipGetLastError();
  });
  return KW_OK;
}

std::unique_ptr<DeviceBatch> host_view(kw_batch* kb) {
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
  static uint32_t dummy;  // (a reordered batch carries no string bytes; the planner reads none)
  std::vector<const uint8_t*> ptr;
  for_each_column(B, [&](PieceKind k, int, const void* p, size_t n) {
    ptr.push_back(k == PK_STR_BYTES && !n ? (const uint8_t*)&dummy : (const uint8_t*)p);
  });
  set_views(D.get(), B, ptr);
  D->verdicts = &dummy;
  D->dev_b = std::move(P);
  return D;
}

}  // namespace kw
