// outcomes.cpp — the grouped outcome count on a resident pass (include/kwgpu.h): kw_batch_outcomes
// sorts the caller's group ids into a row list, counts the last pass's verdict words on the device
// per (group, outcome, column) and reads back only the table; kw_batch_attribute_groups builds the
// dictionary of the rows' metrics attributes on the host workers; the host-reducer diagnostic. The
// arithmetic is outcomes.hpp's, the kernel reports.hip's; capi.cpp folds the table into kw_metrics.
#include "outcomes.hpp"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "knobs.hpp"
#include "lastpass.hpp"
#include "reports.hpp"

namespace kw {
namespace {

int batch_outcomes(kw_batch* b, const uint32_t* row_group, uint32_t ngroups, uint64_t* out) {
  LastPass F(b, LastPass::kAnyPass);
  if (!out || ngroups == 0 || !F.ok()) return KW_E_ARG;
  const uint64_t rows = F.rows;
  const uint32_t npol = F.npol;
  if (rows >> 32) return KW_E_ARG;  // (the sorted list holds u32 rows; a batch's offset columns are u32 too)
  DeviceBatch& D = *F.dev;
  const bool dbg = Knobs::on<KW_BULK_DEBUG>();
  const auto t_start = std::chrono::steady_clock::now();
  // the sorted row list and the unit table, then the rows as the device holds them
  std::vector<uint32_t> start((size_t)ngroups + 1), order((size_t)rows);
  if (!outcome_sort(row_group, rows, ngroups, start.data(), order.data())) return KW_E_ARG;
  memset(out, 0, outcome_table_words(ngroups, npol) * 8);
  if (rows == 0) return KW_OK;
  const uint32_t per = outcome_range_groups(npol, (uint64_t)Knobs::num<KW_OUTCOME_TABLE>());
  const uint32_t nranges = outcome_ranges(ngroups, per);
  std::vector<uint64_t> unit_at((size_t)nranges + 1, 0);  // the first unit of each range
  for (uint32_t k = 0; k < nranges; ++k)
    unit_at[k + 1] = unit_at[k] + outcome_unit_count(start.data(), k * per, (uint32_t)std::min<uint64_t>(ngroups, (uint64_t)(k + 1) * per));
  const uint64_t nunits = unit_at[nranges];
  if (nunits >> 32) return KW_E_ARG;

  if (int rc = F.open()) return rc;
  hipStream_t s = F.s;
  const size_t b_order = (size_t)rows * 4, b_units = (size_t)nunits * sizeof(OutUnit);
  const size_t b_range = outcome_table_words((uint32_t)std::min<uint64_t>(per, ngroups), npol) * 8;
  BlockLease &dorder = F.lease(), &dunits = F.lease(), &dtable = F.lease(), &hin = F.lease(), &htable = F.lease();
  HIPCHK(hin.alloc(host_pool(), D.device, b_order + b_units));
  HIPCHK(htable.alloc(host_pool(), D.device, b_range));
  HIPCHK(dorder.alloc(dev_pool(), D.device, b_order));
  HIPCHK(dunits.alloc(dev_pool(), D.device, b_units));
  HIPCHK(dtable.alloc(dev_pool(), D.device, b_range));
  uint32_t* h_order = (uint32_t*)hin.p;
  OutUnit* h_units = (OutUnit*)((uint8_t*)hin.p + b_order);
  if (D.split) {  // the caller speaks batch rows, the verdict buffer is in device-row order
    const std::vector<uint64_t>& dev_row = D.device_rows();
    if (dev_row.size() != rows) return KW_E_ARG;
    for (uint64_t i = 0; i < rows; ++i) h_order[i] = (uint32_t)dev_row[order[i]];
  } else {
    memcpy(h_order, order.data(), b_order);
  }
  for (uint32_t k = 0; k < nranges; ++k)
    outcome_fill_units(start.data(), k * per, (uint32_t)std::min<uint64_t>(ngroups, (uint64_t)(k + 1) * per), h_units + unit_at[k]);
  const auto t_sorted = std::chrono::steady_clock::now();
  StreamTimer timer(dbg);
  double dev_ms = 0;
  HIPCHK(hipMemcpyAsync(dorder.p, h_order, b_order, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dunits.p, h_units, b_units, hipMemcpyHostToDevice, s));
  // one range at a time through the one table block: zero, count, read back
  for (uint32_t k = 0; k < nranges; ++k) {
    const uint32_t g0 = k * per, g1 = (uint32_t)std::min<uint64_t>(ngroups, (uint64_t)(k + 1) * per);
    if (unit_at[k + 1] == unit_at[k]) continue;  // only empty groups: the zeros are already there
    const size_t bytes = outcome_table_words(g1 - g0, npol) * 8;
    timer.start(s);
    HIPCHK(hipMemsetAsync(dtable.p, 0, bytes, s));
    OutcomeArgs a;
    a.words = D.verdicts;
    a.order = (const uint32_t*)dorder.p;
    a.units = (const OutUnit*)dunits.p + unit_at[k];
    a.table = (uint64_t*)dtable.p;
    a.nunits = (uint32_t)(unit_at[k + 1] - unit_at[k]);
    a.npol = npol;
    a.g0 = g0;
    HIPCHK(launch_outcomes(a, s));
    timer.stop(s);
    HIPCHK(hipMemcpyAsync(htable.p, dtable.p, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    dev_ms += timer.ms();
    memcpy(out + outcome_table_words(g0, npol), htable.p, bytes);
  }
  if (dbg) {
    const std::chrono::duration<double, std::milli> sort = t_sorted - t_start;
    fprintf(stderr, "[kw outcomes] %llu rows x %u, %u groups in %u ranges, %llu units: sort and units %.3f ms on the host, "
            "zero + count %.3f ms on the device, the call %.3f ms\n", (unsigned long long)rows, npol, ngroups, nranges,
            (unsigned long long)nunits, sort.count(), dev_ms, ms_since(t_start));
  }
  return KW_OK;
}

// ---- the attribute dictionary ----
// What Metrics::label_set reads from a row, as one byte string: a raw row reads nothing; any other
// its requestKind.kind ("" when the batch holds none), its operation, and its namespace when it has
// one. The lengths keep (kind, operation) pairs apart whatever bytes they hold.
void attr_key(const Batch& B, uint64_t r, std::string* k) {
  k->clear();
  const uint8_t f = B.req_flags[r];
  if (f & KW_REQ_RAW) {
    k->push_back('r');
    return;
  }
  const bool has_ns = (f & KW_REQ_HAS_NAMESPACE) != 0;
  const std::string_view kind = r < B.rkind.n() ? B.rkind.at(r) : std::string_view(), op = B.op.at(r);
  const uint32_t len[2] = {(uint32_t)kind.size(), (uint32_t)op.size()};
  k->push_back(has_ns ? 'n' : 'a');
  k->append((const char*)len, sizeof(len));
  k->append(kind);
  k->append(op);
  if (has_ns) k->append(B.ns.at(r));
}

constexpr uint64_t kAttrRange = 16384;  // rows of one host-worker task

void build_attr_groups(const Batch& B, kw_batch::AttrGroups* A) {
  struct Part {
    std::vector<std::string> keys;  // the range's distinct keys in order of first appearance
    std::vector<uint64_t> first;    // and their first rows
    std::vector<uint32_t> global;   // their ids in the whole batch (after the merge)
  };
  const uint64_t n = B.n, nparts = (n + kAttrRange - 1) / kAttrRange;
  std::vector<Part> parts((size_t)nparts);
  A->row_group.assign((size_t)n, 0);
  A->first_row.clear();
  HostWorkers::get().run((size_t)nparts, [&](size_t q) {
    Part& P = parts[q];
    std::unordered_map<std::string, uint32_t> ids;
    std::string k;
    for (uint64_t r = q * kAttrRange, e = std::min(n, (q + 1) * kAttrRange); r < e; ++r) {
      attr_key(B, r, &k);
      auto it = ids.find(k);
      if (it == ids.end()) {
        it = ids.emplace(k, (uint32_t)P.keys.size()).first;
        P.keys.push_back(k);
        P.first.push_back(r);
      }
      A->row_group[r] = it->second;  // the range's own id until the merge
    }
  });
  // the ranges in order: a key new to the batch takes the next id, so ids follow first appearance
  std::unordered_map<std::string, uint32_t> ids;
  for (Part& P : parts) {
    P.global.resize(P.keys.size());
    for (size_t i = 0; i < P.keys.size(); ++i) {
      auto it = ids.find(P.keys[i]);
      if (it == ids.end()) {
        it = ids.emplace(std::move(P.keys[i]), (uint32_t)A->first_row.size()).first;
        A->first_row.push_back(P.first[i]);
      }
      P.global[i] = it->second;
    }
  }
  HostWorkers::get().run((size_t)nparts, [&](size_t q) {
    const Part& P = parts[q];
    for (uint64_t r = q * kAttrRange, e = std::min(n, (q + 1) * kAttrRange); r < e; ++r) A->row_group[r] = P.global[A->row_group[r]];
  });
  A->built = true;
}

}  // namespace
}  // namespace kw

extern "C" {

int kw_batch_outcomes(kw_batch* b, const uint32_t* row_group, uint32_t ngroups, uint64_t* out) {
  return kw::batch_outcomes(b, row_group, ngroups, out);
}

int kw_debug_outcome_words(const uint32_t* words, uint64_t rows, uint32_t npol, const uint32_t* row_group, uint32_t ngroups,
                           uint64_t* out) {
  return kw::outcome_reduce(words, rows, npol, row_group, ngroups, out);
}

int kw_batch_attribute_groups(const kw_batch* b, uint32_t* row_group, uint64_t* first_row, size_t cap, uint32_t* ngroups) {
  if (!b || !ngroups) return KW_E_ARG;
  kw_batch::AttrGroups& A = b->attr;
  std::lock_guard<std::mutex> g(A.m);
  if (!A.built) kw::build_attr_groups(b->b, &A);
  *ngroups = (uint32_t)A.first_row.size();
  if (row_group && !A.row_group.empty()) memcpy(row_group, A.row_group.data(), A.row_group.size() * 4);
  if (cap < A.first_row.size() || (!first_row && !A.first_row.empty())) return KW_E_NOSPACE;
  if (!A.first_row.empty()) memcpy(first_row, A.first_row.data(), A.first_row.size() * 8);
  return KW_OK;
}

}  // extern "C"
