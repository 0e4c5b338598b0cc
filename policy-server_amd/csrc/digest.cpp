// digest.cpp — the violation digest on a resident pass (include/kwgpu.h): kw_batch_digest hashes the
// last pass's findings into a table on the device by (column, reason, allowed bit, key), verifies
// every finding against its group's representative, reads back the records, folds the few findings
// the verify launch hands over into them by the exact reducer and sorts; the host-reducer
// diagnostic; the key of one finding. The arithmetic is digest.hpp's, the kernels reports.hip's.
#include "digest.hpp"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "knobs.hpp"
#include "lastpass.hpp"
#include "reports.hpp"

namespace kw {
namespace {

constexpr bool same_col(uint32_t a, uint32_t b) { return a == b; }
static_assert(same_col(DG_NS, S_NS) && same_col(DG_IMG, S_IMG) && same_col(DG_AA, S_AA) && same_col(DG_CAPADD, S_CAPADD) &&
                  same_col(DG_LK, S_LK) && same_col(DG_LV, S_LV) && same_col(DG_NSTR, NSTR),
              "digest.hpp numbers the string columns as kernels.hpp Str");
static_assert(sizeof(DigestSlot) == 24 && sizeof(DigestLeft) == 16 && sizeof(kw_digest_rec) == 24, "digest records");

}  // namespace

// The host batch's columns as the key function reads them (batch rows; members.cpp reads them too).
DigestCols host_cols(const Batch& B) {
  DigestCols C{};
  C.rows = B.n;
  C.nctr = B.containers();
  C.ctr_off = B.ctr_off.data();
  C.lbl_off = B.lbl_off.data();
  C.capadd_off = B.capadd_off.data();
  for (uint32_t m = 0; m < DG_NSTR; ++m) {
    if (m == (uint32_t)S_CAPDROP) continue;  // (no key reads it)
    const StrCol& s = host_str(B, (int)m);
    C.str[m] = DigestStr{s.off.data(), s.bytes.data(), s.n()};
  }
  return C;
}

// The device copy's columns (device rows); a string column that is not resident stays absent.
DigestCols device_cols(const kw_batch* kb) {
  const DeviceBatch& D = *kb->dev;
  const Batch& B = dev_rows(kb);
  DigestCols C{};
  C.rows = B.n;
  C.nctr = B.containers();
  C.ctr_off = D.ctr_off;
  C.lbl_off = D.lbl_off;
  C.capadd_off = D.capadd_off;
  for (uint32_t m = 0; m < DG_NSTR; ++m) {
    if (m == (uint32_t)S_CAPDROP || !((D.loaded >> m) & 1u) || !D.str[m].off || !D.str[m].bytes) continue;
    C.str[m] = DigestStr{D.str[m].off, D.str[m].bytes, host_str(B, (int)m).n()};
  }
  return C;
}

namespace {

int batch_digest(kw_batch* b, kw_digest* out) {
  if (!out) return KW_E_ARG;
  out->n = out->nwide = 0;
  out->findings = 0;
  LastPass F(b, LastPass::kWholeBatch);
  if (!F.ok()) return KW_E_ARG;
  if ((out->cap && !out->recs) || (out->wide_cap && !out->wide)) return KW_E_ARG;
  const uint64_t rows = F.rows;
  const uint32_t npol = F.npol;
  DeviceBatch& D = *F.dev;
  D.digest_ran = true;
  for (uint64_t& v : D.digest_stats) v = 0;
  if (rows == 0) return KW_OK;
  const bool dbg = Knobs::on<KW_BULK_DEBUG>();
  const auto t_start = std::chrono::steady_clock::now();
  const uint64_t budget = (uint64_t)Knobs::num<KW_DIGEST_TABLE>();
  const uint32_t hash_bits = (uint32_t)Knobs::num<KW_DIGEST_HASH_BITS>();
  const uint64_t max_slots = digest_slots(budget, rows * npol), wide_cap = rows;

  if (int rc = F.open()) return rc;
  hipStream_t s = F.s;
  BlockLease &dtable = F.lease(), &dhead = F.lease(), &dwide = F.lease(), &dleft = F.lease(), &drecs = F.lease(),
             &hhead = F.lease(), &hback = F.lease();
  HIPCHK(dtable.alloc(dev_pool(), D.device, (size_t)max_slots * sizeof(DigestSlot)));
  HIPCHK(dhead.alloc(dev_pool(), D.device, sizeof(DigestHead)));
  HIPCHK(dwide.alloc(dev_pool(), D.device, (size_t)wide_cap * 8));
  HIPCHK(dleft.alloc(dev_pool(), D.device, (size_t)kDigestLeftCap * sizeof(DigestLeft)));
  HIPCHK(hhead.alloc(host_pool(), D.device, sizeof(DigestHead)));

  DigestArgs a{};
  a.words = D.verdicts;
  a.cols = device_cols(b);
  a.table = (DigestSlot*)dtable.p;
  a.head = (DigestHead*)dhead.p;
  a.wide = (uint64_t*)dwide.p;
  a.left = (DigestLeft*)dleft.p;
  a.wide_cap = wide_cap;
  a.left_cap = kDigestLeftCap;
  a.hash_bits = hash_bits;
  a.npol = npol;
  a.loaded = D.loaded;
  // (a split batch: the verdict buffer is in device-row order, first_row speaks batch rows)
  if (int rc = upload_row_maps(F, &a.d2b, &a.b2d)) return rc;
  const double prep_ms = ms_since(t_start);

  const DigestCols H = host_cols(b->b);
  std::vector<kw_digest_rec> recs;
  std::vector<uint64_t> wide;
  DigestAcc left;  // the leftovers' groups: none of them is a group of the table (a group has one tag, a tag one slot)
  uint64_t findings = 0, nleft = 0, cuts = 0, slots = 0;
  double count_ms = 0, verify_ms = 0, gather_ms = 0, back_ms = 0;
  StreamTimer t_count(dbg), t_verify(dbg), t_gather(dbg);
  DigestHead* hh = (DigestHead*)hhead.p;

  auto run = [&](uint32_t c0, uint32_t c1) -> int {
    a.c0 = c0;
    a.c1 = c1;
    a.nslots = digest_slots(budget, rows * (uint64_t)(c1 - c0));
    slots = std::max(slots, a.nslots);
    HIPCHK(hipMemsetAsync(dtable.p, 0, (size_t)a.nslots * sizeof(DigestSlot), s));
    HIPCHK(hipMemsetAsync(dhead.p, 0, sizeof(DigestHead), s));
    t_count.start(s);
    HIPCHK(launch_digest_count(a, s));
    t_count.stop(s);
    // (the count's status first: a range that must be cut is not verified)
    HIPCHK(hipMemcpyAsync(hh, dhead.p, sizeof(DigestHead), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    count_ms += t_count.ms();
    if (hh->missing) return KW_E_ARG;
    if (int rc = digest_range_status(*hh, a.nslots, wide_cap, kDigestLeftCap)) {
      ++cuts;
      return rc;
    }
    t_verify.start(s);
    HIPCHK(launch_digest_verify(a, s));
    t_verify.stop(s);
    HIPCHK(hipMemcpyAsync(hh, dhead.p, sizeof(DigestHead), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    verify_ms += t_verify.ms();
    if (int rc = digest_range_status(*hh, a.nslots, wide_cap, kDigestLeftCap)) {  // (the leftover list)
      ++cuts;
      return rc;
    }
    const DigestHead h = *hh;
    const size_t b_rec = (size_t)h.nclaimed * sizeof(kw_digest_rec), b_left = (size_t)h.nleft * sizeof(DigestLeft),
                 b_wide = (size_t)h.nwide * 8;
    HIPCHK(hback.alloc(host_pool(), D.device, std::max<size_t>(b_rec + b_left + b_wide, 64)));
    if (h.nclaimed) {
      HIPCHK(drecs.alloc(dev_pool(), D.device, b_rec));
      a.recs = (kw_digest_rec*)drecs.p;
      a.rec_cap = h.nclaimed;
      t_gather.start(s);
      HIPCHK(launch_digest_gather(a, s));
      t_gather.stop(s);
    }
    const auto t_back = std::chrono::steady_clock::now();
    uint8_t* hb = (uint8_t*)hback.p;
    HIPCHK(hipMemcpyAsync(hh, dhead.p, sizeof(DigestHead), hipMemcpyDeviceToHost, s));
    if (b_rec) HIPCHK(hipMemcpyAsync(hb, drecs.p, b_rec, hipMemcpyDeviceToHost, s));
    if (b_left) HIPCHK(hipMemcpyAsync(hb + b_rec, dleft.p, b_left, hipMemcpyDeviceToHost, s));
    if (b_wide) HIPCHK(hipMemcpyAsync(hb + b_rec + b_left, dwide.p, b_wide, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h.nclaimed) gather_ms += t_gather.ms();
    back_ms += ms_since(t_back);
    if (hh->nrec > h.nclaimed) return KW_E_ENGINE;
    const kw_digest_rec* r = (const kw_digest_rec*)hb;
    recs.insert(recs.end(), r, r + hh->nrec);
    const DigestLeft* l = (const DigestLeft*)(hb + b_rec);
    for (uint64_t i = 0; i < h.nleft; ++i) {
      const uint64_t drow = l[i].pair / npol;
      digest_add(&left, H, D.split ? D.perm[drow] : drow, (uint32_t)(l[i].pair % npol), npol, l[i].word);
    }
    const uint64_t* w = (const uint64_t*)(hb + b_rec + b_left);
    for (uint64_t i = 0; i < h.nwide; ++i) wide.push_back((D.split ? D.perm[w[i] / npol] : w[i] / npol) * npol + w[i] % npol);
    findings += h.findings;
    nleft += h.nleft;
    return KW_OK;
  };
  uint32_t ranges = 0;
  const int rc = digest_ranges(0, npol, run, &ranges);
  D.digest_stats[0] = ranges;
  D.digest_stats[1] = nleft;
  D.digest_stats[2] = slots;
  D.digest_stats[3] = cuts;
  if (rc != KW_OK) return rc;
  const size_t from_table = recs.size();
  digest_records(left, &recs);
  const int erc = digest_emit(&recs, &wide, findings, out);
  if (dbg)
    fprintf(stderr, "[kw digest] %llu rows x %u, %llu findings, %zu groups (%zu from the table, %llu leftovers), %zu wide, %u ranges "
            "(%llu cut), %llu slots: prepare %.3f ms on the host, count %.3f ms verify %.3f ms gather %.3f ms on the device, "
            "read-back %.3f ms, the call %.3f ms\n", (unsigned long long)rows, npol, (unsigned long long)findings, recs.size(),
            from_table, (unsigned long long)nleft, wide.size(), ranges, (unsigned long long)cuts, (unsigned long long)slots, prep_ms,
            count_ms, verify_ms, gather_ms, back_ms, ms_since(t_start));
  return erc;
}

}  // namespace
}  // namespace kw

extern "C" {

int kw_batch_digest(kw_batch* b, kw_digest* out) { return kw::batch_digest(b, out); }

int kw_debug_digest_words(const kw_batch* b, const uint32_t* words, uint64_t rows, uint32_t npol, kw_digest* out) {
  if (!b || !out || npol == 0 || rows > b->b.n || (rows && !words)) return KW_E_ARG;
  if ((out->cap && !out->recs) || (out->wide_cap && !out->wide)) return KW_E_ARG;
  const kw::DigestCols H = kw::host_cols(b->b);
  kw::DigestAcc acc;
  kw::digest_reduce(H, words, rows, npol, &acc);
  std::vector<kw_digest_rec> recs;
  kw::digest_records(acc, &recs);
  return kw::digest_emit(&recs, &acc.wide, acc.findings, out);
}

int kw_batch_finding_key(const kw_batch* b, uint64_t row, uint32_t word, char* buf, size_t cap, size_t* need, size_t* split) {
  if (!b || !need || !split || row >= b->b.n || !kw::digest_finding(word) || kw::digest_wide(word)) return KW_E_ARG;
  const kw::DigestKey k = kw::digest_key(kw::host_cols(b->b), row, word);
  *need = (size_t)k.n0 + k.n1;
  *split = kw::digest_kind(KW_REASON(word)) == kw::DK_LKV ? (size_t)k.n0 : *need;
  if (*need > cap || (*need && !buf)) return KW_E_NOSPACE;
  if (k.n0) memcpy(buf, k.p0, k.n0);
  if (k.n1) memcpy(buf + k.n0, k.p1, k.n1);
  return KW_OK;
}

int kw_debug_digest_stats(const kw_batch* b, uint64_t* out) {
  if (!b || !out || !b->dev || !b->dev->digest_ran) return KW_E_ARG;
  for (int i = 0; i < 4; ++i) out[i] = b->dev->digest_stats[i];
  return KW_OK;
}

}  // extern "C"
