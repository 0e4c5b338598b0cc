// members.cpp — the digest's drill-down on a resident pass (include/kwgpu.h):
// kw_batch_digest_members builds the selection table of the named groups on the host, checks every
// record's word against the pass and walks the words once on the device, reads back the per-group
// counts and the members found, and orders them by (group, row) on the host workers; the
// host-reducer diagnostic. The arithmetic is members.hpp's, the kernels reports.hip's.
#include "members.hpp"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "knobs.hpp"
#include "lastpass.hpp"
#include "reports.hpp"

namespace kw {
namespace {

static_assert(sizeof(MemberSlot) == 32 && sizeof(MemberEntry) == 16 && sizeof(MembersHead) == 16, "members records");

int batch_members(kw_batch* b, const kw_digest_rec* groups, size_t ngroups, kw_members* out) {
  if (!out) return KW_E_ARG;
  out->n = 0;
  LastPass F(b, LastPass::kWholeBatch);
  if (!F.ok()) return KW_E_ARG;
  const uint64_t rows = F.rows;
  const uint32_t npol = F.npol;
  DeviceBatch& D = *F.dev;
  if (!members_out_ok(groups, ngroups, out)) return KW_E_ARG;
  if (ngroups == 0) {
    if (out->off) out->off[0] = 0;
    return KW_OK;
  }
  const bool dbg = Knobs::on<KW_BULK_DEBUG>();
  const auto t_start = std::chrono::steady_clock::now();
  const uint32_t hash_bits = (uint32_t)Knobs::num<KW_DIGEST_HASH_BITS>();

  // the selection table from the host batch's columns; its representatives in device rows
  MembersTable T;
  const DigestCols H = host_cols(b->b);
  if (int rc = members_table(H, groups, ngroups, rows, npol, hash_bits, D.split ? D.device_rows().data() : nullptr, &T)) return rc;
  const DigestCols C = device_cols(b);
  const uint32_t have = resident_mask(C);
  if (members_need(groups, ngroups) & ~have) return KW_E_ARG;  // a key column that is not resident
  const uint64_t pairs = rows * npol, list_cap = std::min<uint64_t>(out->cap, pairs);
  const double table_ms = ms_since(t_start);

  if (int rc = F.open()) return rc;
  hipStream_t s = F.s;
  BlockLease &din = F.lease(), &dacc = F.lease(), &dlist = F.lease(), &hin = F.lease(), &hacc = F.lease(), &hlist = F.lease();
  // in: [slots][column masks]; acc: [head][counts]
  const size_t b_slots = T.slots.size() * sizeof(MemberSlot), b_in = b_slots + (size_t)npol * 8;
  const size_t b_acc = sizeof(MembersHead) + ngroups * 8;
  HIPCHK(hin.alloc(host_pool(), D.device, b_in));
  HIPCHK(din.alloc(dev_pool(), D.device, b_in));
  HIPCHK(dacc.alloc(dev_pool(), D.device, b_acc));
  HIPCHK(hacc.alloc(host_pool(), D.device, b_acc));
  HIPCHK(dlist.alloc(dev_pool(), D.device, (size_t)std::max<uint64_t>(list_cap, 1) * sizeof(MemberEntry)));
  uint8_t* hi = (uint8_t*)hin.p;
  memcpy(hi, T.slots.data(), b_slots);
  memcpy(hi + b_slots, T.colmask.data(), (size_t)npol * 8);
  HIPCHK(hipMemcpyAsync(din.p, hin.p, b_in, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(dacc.p, 0, b_acc, s));

  MembersArgs a{};
  a.words = D.verdicts;
  a.cols = C;
  a.table = (const MemberSlot*)din.p;
  a.colmask = (const uint64_t*)((const uint8_t*)din.p + b_slots);
  // (a split batch: the verdict buffer is in device-row order, the members speak batch rows)
  if (int rc = upload_row_maps(F, &a.d2b)) return rc;
  a.head = (MembersHead*)dacc.p;
  a.counts = (uint64_t*)((uint8_t*)dacc.p + sizeof(MembersHead));
  a.list = (MemberEntry*)dlist.p;
  a.nslots = T.slots.size();
  a.list_cap = list_cap;
  a.hash_bits = hash_bits;
  a.npol = npol;
  a.loaded = have;
  const double prep_ms = ms_since(t_start);

  StreamTimer t_check(dbg), t_walk(dbg), t_acc(dbg), t_list(dbg);
  t_check.start(s);
  HIPCHK(launch_members_check(a, s));
  t_check.stop(s);
  t_walk.start(s);
  HIPCHK(launch_members_walk(a, s));
  t_walk.stop(s);
  t_acc.start(s);
  HIPCHK(hipMemcpyAsync(hacc.p, dacc.p, b_acc, hipMemcpyDeviceToHost, s));
  t_acc.stop(s);
  HIPCHK(hipStreamSynchronize(s));
  const double check_ms = t_check.ms(), walk_ms = t_walk.ms();
  const MembersHead head = *(const MembersHead*)hacc.p;
  if (head.bad) return KW_E_ARG;  // a record of another pass
  const uint64_t* counts = (const uint64_t*)((const uint8_t*)hacc.p + sizeof(MembersHead));
  const int orc = members_offsets(counts, ngroups, out);
  if ((uint64_t)out->n != head.nlist) return KW_E_ENGINE;
  double back_ms = t_acc.ms(), order_ms = 0;
  if (orc == KW_OK && out->n) {
    const size_t b_list = out->n * sizeof(MemberEntry);
    HIPCHK(hlist.alloc(host_pool(), D.device, b_list));
    t_list.start(s);
    HIPCHK(hipMemcpyAsync(hlist.p, dlist.p, b_list, hipMemcpyDeviceToHost, s));
    t_list.stop(s);
    HIPCHK(hipStreamSynchronize(s));
    back_ms += t_list.ms();
    const auto t_order = std::chrono::steady_clock::now();
    const auto workers = [](size_t n, const std::function<void(size_t)>& fn) { HostWorkers::get().run(n, fn); };
    if (!members_order((const MemberEntry*)hlist.p, out->off, ngroups, out->rows, out->words, workers)) return KW_E_ENGINE;
    order_ms = ms_since(t_order);
  }
  if (dbg)
    fprintf(stderr, "[kw members] %llu rows x %u, %zu groups named, %llu slots, %zu members%s: table %.3f ms and upload staging %.3f ms "
            "on the host, check %.3f ms walk %.3f ms on the device, read-back %.3f ms (the copies, by events), ordering %.3f ms on the host, the call %.3f ms\n",
            (unsigned long long)rows, npol, ngroups, (unsigned long long)a.nslots, out->n, orc == KW_OK ? "" : " (more than cap)",
            table_ms, prep_ms - table_ms, check_ms, walk_ms, back_ms, order_ms, ms_since(t_start));
  return orc;
}

}  // namespace
}  // namespace kw

extern "C" {

int kw_batch_digest_members(kw_batch* b, const kw_digest_rec* groups, size_t ngroups, kw_members* out) {
  return kw::batch_members(b, groups, ngroups, out);
}

int kw_debug_digest_members_words(const kw_batch* b, const uint32_t* words, uint64_t rows, uint32_t npol,
                                  const kw_digest_rec* groups, size_t ngroups, kw_members* out) {
  if (!out) return KW_E_ARG;
  out->n = 0;
  if (!b || npol == 0 || rows > b->b.n || (rows && !words) || (rows >> 32)) return KW_E_ARG;
  if (!kw::members_out_ok(groups, ngroups, out)) return KW_E_ARG;
  std::vector<uint64_t> counts;
  std::vector<kw::MemberEntry> list;
  if (int rc = kw::members_reduce(kw::host_cols(b->b), words, rows, npol, groups, ngroups, &counts, &list)) return rc;
  if (ngroups == 0) {
    if (out->off) out->off[0] = 0;
    return KW_OK;
  }
  if (int rc = kw::members_offsets(counts.data(), ngroups, out)) return rc;
  return kw::members_order(list.data(), out->off, ngroups, out->rows, out->words, kw::MembersSerial{}) ? KW_OK : KW_E_ENGINE;
}

}  // extern "C"
