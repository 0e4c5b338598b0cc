// members.cpp — the digest's drill-down on a resident pass (include/kwgpu.h):
// kw_batch_digest_members builds the selection table of the named groups on the host, checks every
// record's word against the pass and walks the words once on the device, reads back the per-group
// counts and the members found, and orders them by (group, row) on the host workers; the
// host-reducer diagnostic. The arithmetic is members.hpp's, the kernels kernels.hip's.
#include "members.hpp"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "devbatch.hpp"
#include "kernels.hpp"
#include "knobs.hpp"
#include "pass.hpp"

namespace kw {
namespace {

static_assert(sizeof(MemberSlot) == 32 && sizeof(MemberEntry) == 16 && sizeof(MembersHead) == 16, "members records");

// Declared after the leases a call holds: the stream is drained before any block returns to its pool,
// on the error returns too.
struct Drain {
  hipStream_t s;
  ~Drain() { (void)hipStreamSynchronize(s); }
};

double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

size_t up16(size_t n) { return (n + 15u) & ~(size_t)15u; }

int batch_members(kw_batch* b, const kw_digest_rec* groups, size_t ngroups, kw_members* out) {
  if (!out) return KW_E_ARG;
  out->n = 0;
  uint64_t rows = 0;
  uint32_t npol = 0;
  if (kw_batch_last_pass(b, &rows, &npol) != KW_OK) return KW_E_ARG;
  DeviceBatch& D = *b->dev;
  if (D.last_rows_mode || (rows >> 32) || rows != b->b.n) return KW_E_ARG;
  if (D.split && D.perm.size() != rows) return KW_E_ARG;
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
  uint32_t have = 0;
  for (uint32_t m = 0; m < DG_NSTR; ++m)
    if (C.str[m].off) have |= 1u << m;
  if (members_need(groups, ngroups) & ~have) return KW_E_ARG;  // a key column that is not resident
  const uint64_t pairs = rows * npol, list_cap = std::min<uint64_t>(out->cap, pairs);
  const double table_ms = ms_since(t_start);

  HIPCHK(hipSetDevice(D.device));
  hipStream_t s = D.cur ? D.cur : D.stream;
  BlockLease din, dacc, dlist, hin, hacc, hlist;
  Drain drain{s};
  // in: [slots][column masks][row map]; acc: [head][counts]
  const size_t b_slots = T.slots.size() * sizeof(MemberSlot), b_mask = up16((size_t)npol * 8),
               b_map = D.split ? up16((size_t)rows * 4) : 0, b_in = b_slots + b_mask + b_map;
  const size_t b_acc = sizeof(MembersHead) + ngroups * 8;
  HIPCHK(hin.alloc(host_pool(), D.device, b_in));
  HIPCHK(din.alloc(dev_pool(), D.device, b_in));
  HIPCHK(dacc.alloc(dev_pool(), D.device, b_acc));
  HIPCHK(hacc.alloc(host_pool(), D.device, b_acc));
  HIPCHK(dlist.alloc(dev_pool(), D.device, (size_t)std::max<uint64_t>(list_cap, 1) * sizeof(MemberEntry)));
  uint8_t* hi = (uint8_t*)hin.p;
  memcpy(hi, T.slots.data(), b_slots);
  memcpy(hi + b_slots, T.colmask.data(), (size_t)npol * 8);
  if (D.split) {  // the verdict buffer is in device-row order, the members speak batch rows
    uint32_t* m = (uint32_t*)(hi + b_slots + b_mask);
    for (uint64_t i = 0; i < rows; ++i) m[i] = (uint32_t)D.perm[i];
  }
  HIPCHK(hipMemcpyAsync(din.p, hin.p, b_in, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(dacc.p, 0, b_acc, s));

  MembersArgs a{};
  a.words = D.verdicts;
  a.cols = C;
  a.table = (const MemberSlot*)din.p;
  a.colmask = (const uint64_t*)((const uint8_t*)din.p + b_slots);
  a.d2b = D.split ? (const uint32_t*)((const uint8_t*)din.p + b_slots + b_mask) : nullptr;
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
