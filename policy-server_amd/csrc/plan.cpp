// plan.cpp — planning of one pass (plan.hpp). A planning translation unit: every KW_* setting it
// reads goes through PlanKnobs, so it is part of the plan cache's key (knobs.hpp kw_knob_hash) by construction.
#define KW_PLANNING_TU
#include "plan.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>

#include "groups.hpp"
#include "groupvm.hpp"
#include "knobs.hpp"
#include "slots.hpp"

namespace kw {

// Tile schedule of a launch of `ntiles` tiles over `grid` workgroups: the dynamic one (per-XCD
// counters from a slot's third tile on, kernels.hip) only where a workgroup runs more than 16 tiles,
// so that drift between workgroups has room to build up; below that the launch is strided, with a
// counter-drawn tail where sched_static_rounds (below) gives it one. KW_SCHED=static / dynamic
// forces one. Tables read from global memory (C6) make tile costs vary with the caches: there the
// dynamic schedule pays from 4 tiles a workgroup (C6 at 15: -2 %).
// The thresholds are r05's (profiles/r05_sched_ab.txt: strided C4 -2.4 %, C2 -6 %, C1 -40 %, a
// 64k-request shard -47 %; dynamic C5 -7 %, C6 -2 %, C3 -2 %). What r05 measured as the counters'
// cost was mostly not the fetches: r09 found a device-scope fence at every workgroup's end and a
// wait on each fetch at the top of its tile, and removed both (profiles/r09_sched_tail_ab.txt:
// C4 forced dynamic 0.247 -> 0.223 ms at 1M, 0.063 -> 0.042 ms at 125k, against 0.237 and 0.041
// strided). The thresholds have not been measured again since.
bool sched_dynamic(uint64_t ntiles, uint32_t grid, bool lds_tables) {
  const char* e = PlanKnobs::str<KW_SCHED>();
  if (!strcmp(e, "static")) return false;
  if (!strcmp(e, "dynamic")) return true;
  return ntiles > (lds_tables ? 16ull : 4ull) * std::max<uint32_t>(grid, 1);
}

// Static rounds S of a launch of `ndesc` descriptors (the launch's actual count, not the planner's
// estimate) over `grid` workgroups, whose plan chose the dynamic schedule or not (`dyn`,
// sched_dynamic): -1 for the strided schedule with no counter, else the S the kernel is handed with
// the counters (EvalArgs::sched_static).
// A launch that sched_dynamic leaves strided still finishes unevenly: its slots run at different
// speeds, and with every tile assigned up front the launch lasts as long as its slowest slot while
// the others stand idle (C4 at 1M under the timing build: 10.3 % of slot-time; with a tail 3.0 %). So with
// q >= kSchedTailMinRounds whole rounds (kernels.hpp tile_whole_rounds) it runs its first
// q - kSchedTail rounds strided and draws the tail from the counters: about kSchedTail + 2 fetches
// a workgroup, spread out because slots reach the tail at different times.
// The rounds are those of the grid really launched (kernels.hpp tile_launch_grid), which the kernel's
// own arithmetic uses.
// Same-box A/B against the parent (profiles/r09_sched_tail_ab.txt): C4 at 1M (15 rounds) -6 %,
// at 500k (7) -6 %, C2 -5 %, C3 -8 %; tails of 2, 3 and 4 rounds and the fully dynamic schedule
// measure alike there and a tail of 1 half as good, so the shortest that works; at 6 rounds the
// tail is level with the strided schedule and at 4 and 5 rounds 1-2 % behind it, so those launches,
// the multi-GPU shards of a few rounds and the bulk path's 4-round chunks stay purely strided.
// KW_SCHED_TAIL=T forces a tail of T rounds on every launch that has two static rounds left beside
// it (q >= T + 2: the kernel fixes a slot's first two tiles before its first fetch);
// KW_SCHED_TAIL=0 is the choice of sched_dynamic alone; KW_SCHED=static / dynamic force theirs.
constexpr uint32_t kSchedTail = 2, kSchedTailMinRounds = 7;
int sched_static_rounds(uint64_t ndesc, uint32_t grid, bool dyn) {
  const int forced = PlanKnobs::num<KW_SCHED_TAIL>();
  const int today = dyn ? 2 : -1;
  const char* e = PlanKnobs::str<KW_SCHED>();
  if (!strcmp(e, "static") || !strcmp(e, "dynamic") || forced == 0 || !grid) return today;
  const uint64_t q = tile_whole_rounds(ndesc, grid);
  if (forced > 0) return q >= (uint64_t)forced + 2 ? (int)std::min<uint64_t>(q - (uint64_t)forced, INT_MAX) : today;
  if (dyn || q < kSchedTailMinRounds) return today;
  return (int)std::min<uint64_t>(q - kSchedTail, INT_MAX);
}

namespace {

// Tile height of a split batch's heavy region (KW_HEAVY_ROWS, A/B knob; 0: planned like any batch).
uint32_t heavy_rows() { return (uint32_t)PlanKnobs::num<KW_HEAVY_ROWS>(); }

// Requests per tile of the tile kernel forced by KW_SLOT_ROWS (8..255: tile-local owners are u8;
// A/B knob, read per pass: tests switch it between passes), 0 = chosen per batch (pick_rows:
// kSlotRows, or taller tiles where they keep enough workgroups per CU).
uint32_t slot_rows_forced() { return (uint32_t)PlanKnobs::num<KW_SLOT_ROWS>(); }

// The next-tile L2 prefetch at run time (KW_L2_PREFETCH=1, A/B knob; the kernel carries its code when
// built with KW_PREFETCH). Off: running it costs C4 3.5 % and C6 3.8 % (r04 same-box A/B), while the
// kernel built with the code present and the plan leaving it off was 2 % faster on C2 / C3 / C4
// than the kernel built without it (profiles/r04_prefetch_ab.txt).
bool l2_prefetch() { return KW_PREFETCH && PlanKnobs::on<KW_L2_PREFETCH>(); }

}  // namespace

// Entity range [g0, g1) of string column m for requests [r0, r1).
void str_range(const Batch& B, int m, uint64_t r0, uint64_t r1, uint64_t* g0, uint64_t* g1) {
  switch (m) {
    case S_NS: *g0 = r0; *g1 = r1; break;
    case S_CAPADD: *g0 = B.capadd_off[B.ctr_off[r0]]; *g1 = B.capadd_off[B.ctr_off[r1]]; break;
    case S_CAPDROP: *g0 = B.capdrop_off[B.ctr_off[r0]]; *g1 = B.capdrop_off[B.ctr_off[r1]]; break;
    case S_LK: case S_LV: *g0 = B.lbl_off[r0]; *g1 = B.lbl_off[r1]; break;
    default: *g0 = B.ctr_off[r0]; *g1 = B.ctr_off[r1]; break;
  }
}

namespace {

constexpr uint32_t kTableBudget = 64 * 1024;   // classifiers + chunk records staged per workgroup
constexpr uint32_t kTileLdsBudget = 160 * 1024;  // tile-kernel LDS per workgroup (gfx950: 160 KB per CU)
constexpr uint32_t kMaxTileEntities = 60000;    // per-request indices in a tile stay below ARG's 65535
constexpr double kTileQuantiles[] = {1.0, 0.99995, 0.9999, 0.9995, 0.999, 0.998};  // capacity candidates

// What each tile of `rows` requests of rows [lo, hi) stages: entity counts and the 16-B aligned byte
// span of each string column.
std::vector<TileStats> tile_needs(const Batch& B, uint32_t rows, uint32_t stride, uint64_t lo, uint64_t hi) {
  const uint64_t ntiles_all = (hi - lo + rows - 1) / rows;
  const uint64_t ntiles = (ntiles_all + stride - 1) / stride;  // sampled tiles: every stride-th
  std::vector<TileStats> v(ntiles);
  // tiles in ranges of 256 on the host workers (each tile's reads are cache misses: 1M requests
  // take ~3 ms on one thread per tile height)
  constexpr uint64_t kRange = 256;
  HostWorkers::get().run((size_t)((ntiles + kRange - 1) / kRange), [&](size_t q) {
  for (uint64_t j = q * kRange, t1 = std::min<uint64_t>(ntiles, (q + 1) * kRange); j < t1; ++j) {
    const uint64_t t = j * stride;
    const uint64_t r0 = lo + t * rows, r1 = std::min<uint64_t>(hi, lo + (t + 1) * rows);
    TileStats& st = v[j];
    st.ctr = B.ctr_off[r1] - B.ctr_off[r0];
    st.lbl = B.lbl_off[r1] - B.lbl_off[r0];
    st.kadd = B.capadd_off[B.ctr_off[r1]] - B.capadd_off[B.ctr_off[r0]];
    st.kdrop = B.capdrop_off[B.ctr_off[r1]] - B.capdrop_off[B.ctr_off[r0]];
    for (int m = 0; m < (int)NSTR; ++m) {
      const StrCol& c = host_str(B, m);
      uint64_t g0, g1;
      str_range(B, m, r0, r1, &g0, &g1);
      st.bytes[m] = ((c.off[g1] + 15u) & ~15u) - (c.off[g0] & ~15u);
    }
  }
  });
  return v;
}

// Per-dimension quantile of the tile needs (quantile 1 = the batch maximum).
TileStats tile_quantile(const std::vector<TileStats>& need, double quantile) {
  TileStats st;
  if (need.empty()) return st;
  const uint64_t n = need.size();
  const uint64_t q = quantile >= 1.0 ? n - 1 : (uint64_t)(quantile * (double)(n - 1));
  std::vector<uint32_t> v(n);
  auto quant = [&](auto f) {
    for (uint64_t t = 0; t < n; ++t) v[t] = f(need[t]);
    std::nth_element(v.begin(), v.begin() + (long)q, v.end());
    return v[q];
  };
  st.ctr = quant([](const TileStats& x) { return x.ctr; });
  st.lbl = quant([](const TileStats& x) { return x.lbl; });
  st.kadd = quant([](const TileStats& x) { return x.kadd; });
  st.kdrop = quant([](const TileStats& x) { return x.kdrop; });
  for (int m = 0; m < (int)NSTR; ++m) st.bytes[m] = quant([m](const TileStats& x) { return x.bytes[m]; });
  return st;
}

// All the capacity-candidate quantiles at once (kTileQuantiles order): per dimension one selection
// at the lowest quantile and a sort of the tail above it (the candidates are all >= 0.998: a few
// dozen values of a 1M-request batch's 15k tiles), dimensions on the host workers.
std::vector<TileStats> tile_quantiles(const std::vector<TileStats>& need, const double* qs, size_t nq) {
  std::vector<TileStats> out(nq);
  if (need.empty() || nq == 0) return out;
  const uint64_t n = need.size();
  std::vector<uint64_t> qi(nq);
  uint64_t qmin = n - 1;
  for (size_t k = 0; k < nq; ++k) {
    qi[k] = qs[k] >= 1.0 ? n - 1 : (uint64_t)(qs[k] * (double)(n - 1));
    qmin = std::min(qmin, qi[k]);
  }
  constexpr int kDims = 4 + (int)NSTR;
  auto dim = [](const TileStats& x, int d) -> uint32_t {
    return d == 0 ? x.ctr : d == 1 ? x.lbl : d == 2 ? x.kadd : d == 3 ? x.kdrop : x.bytes[d - 4];
  };
  auto put = [](TileStats& x, int d, uint32_t v) {
    if (d == 0) x.ctr = v;
    else if (d == 1) x.lbl = v;
    else if (d == 2) x.kadd = v;
    else if (d == 3) x.kdrop = v;
    else x.bytes[d - 4] = v;
  };
  auto one_dim = [&](size_t di) {
    const int d = (int)di;
    std::vector<uint32_t> v(n);
    for (uint64_t t = 0; t < n; ++t) v[t] = dim(need[t], d);
    std::nth_element(v.begin(), v.begin() + (long)qmin, v.end());
    std::sort(v.begin() + (long)qmin, v.end());
    for (size_t k = 0; k < qi.size(); ++k) put(out[k], d, v[qi[k]]);
  };
  if (n < 8192) {  // a small batch (kwhost's micro-batches): inline, no worker wake-up
    for (int d = 0; d < kDims; ++d) one_dim((size_t)d);
  } else {
    HostWorkers::get().run(kDims, one_dim);
  }
  return out;
}

}  // namespace

// The wide groups among the pass's columns (plan->wide): column ids are the output column
// (all pairs) or the rows-mode column code ((chunk << 16) | column, as rowcol holds).
void plan_wide_groups(const Env& E, const std::vector<int32_t>& list, const std::vector<uint32_t>* rows_code,
                      int origin, PassPlan* plan) {
  PassPlan::Wide& W = plan->wide;
  W = PassPlan::Wide{};
  std::map<int32_t, uint32_t> mcol, aux_of;
  auto member_col = [&](int32_t m) {
    auto it = mcol.find(m);
    if (it == mcol.end()) {
      it = mcol.emplace(m, (uint32_t)W.members.size()).first;
      W.members.push_back(m);
    }
    return it->second;
  };
  // a group member that is split: its word is combined from its parts' words where the group
  // reads it (before, the member pass left a placeholder and the group rejected)
  auto split_member = [&](int32_t m) -> uint32_t {
    auto it = aux_of.find(m);
    if (it != aux_of.end()) return it->second;
    const PolicyRec& M = E.pol[(size_t)m];
    WideGroupArgs a;
    memset(&a, 0, sizeof(a));
    while (W.progs.size() % 4) W.progs.push_back(0);
    a.prog_off = (uint32_t)W.progs.size();
    a.prog_len = (uint32_t)(M.part_off.size() * 4);
    W.progs.insert(W.progs.end(), (const uint8_t*)M.part_off.data(), (const uint8_t*)(M.part_off.data() + M.part_off.size()));
    a.kind = M.family == FAM_CAPABILITIES ? 3u : 2u;
    a.nmem = (uint32_t)M.parts.size();
    a.okw = finish_word(M.mode, M.allowed_to_mutate, origin, 0, 0, false);
    a.mutw = finish_word(M.mode, M.allowed_to_mutate, origin, 0, 0, true);
    a.rejb = finish_word(M.mode, M.allowed_to_mutate, origin, 1, 0, false) & ~0xff00u;
    std::vector<uint32_t> cols;
    for (int32_t q : M.parts) cols.push_back(member_col(q));
    a.midx_off = (uint32_t)W.midx.size();
    W.midx.insert(W.midx.end(), cols.begin(), cols.end());
    const uint32_t k = (uint32_t)W.aux.size();
    W.aux.push_back(a);
    aux_of.emplace(m, k);
    return k;
  };
  for (uint32_t j = 0; j < (uint32_t)list.size(); ++j) {
    const PolicyRec& P = E.pol[(size_t)list[j]];
    const bool split = !P.parts.empty() && !P.init_error;
    if (!split && (!P.is_group || P.init_error || !P.prog.valid || P.prog.eval_error || !P.prog.wide)) continue;
    WideGroupArgs g;
    memset(&g, 0, sizeof(g));
    while (W.progs.size() % 4) W.progs.push_back(0);
    g.prog_off = (uint32_t)W.progs.size();
    if (split) {  // the parts' index offsets (u32 each)
      g.prog_len = (uint32_t)(P.part_off.size() * 4);
      W.progs.insert(W.progs.end(), (const uint8_t*)P.part_off.data(), (const uint8_t*)(P.part_off.data() + P.part_off.size()));
    } else {
      g.prog_len = (uint32_t)P.prog.code.size();
      W.progs.insert(W.progs.end(), P.prog.code.begin(), P.prog.code.end());
    }
    g.col = rows_code ? (*rows_code)[j] : j;
    const std::vector<int32_t>& mem = split ? P.parts : P.members;
    g.nmem = (uint32_t)mem.size();
    std::vector<uint32_t> cols;
    for (int32_t m : mem) {
      const PolicyRec& M = E.pol[(size_t)m];
      cols.push_back(!split && !M.parts.empty() && !M.init_error ? kSplitMember | split_member(m) : member_col(m));
    }
    g.midx_off = (uint32_t)W.midx.size();
    W.midx.insert(W.midx.end(), cols.begin(), cols.end());
    if (split) {  // a plain policy's words (slotplan.cpp CK_PLAIN), the reason and argument from its parts
      g.kind = P.family == FAM_CAPABILITIES ? 3u : 2u;
      g.okw = finish_word(P.mode, P.allowed_to_mutate, origin, 0, 0, false);
      g.mutw = finish_word(P.mode, P.allowed_to_mutate, origin, 0, 0, true);
      g.rejb = finish_word(P.mode, P.allowed_to_mutate, origin, 1, 0, false) & ~0xff00u;
      g.cause_words = 0;
    } else {
      g.okw = finish_word(P.mode, 0, origin, 0, 0, false);
      g.rejb = finish_word(P.mode, 0, origin, KW_R_GROUP, kArgWide, false);
      g.errw = finish_word(P.mode, 0, origin, KW_R_GROUP_EXPR, 0, false);
      g.kind = P.prog.script ? 1u : 0u;
      g.cause_words = (g.nmem + 63u) / 64u;
    }
    // all pairs: every wide column has its own words in a row; rows mode: a row has one column
    g.cause_off = rows_code ? 0u : W.cause_stride;
    W.cause_stride = rows_code ? std::max(W.cause_stride, g.cause_words) : W.cause_stride + g.cause_words;
    if (!split)
      W.stack_words = std::max<uint32_t>(W.stack_words, P.prog.script ? (uint32_t)run_script_words(P.prog.code.data())
                                                                       : (P.prog.depth + 63u) / 64u);
    W.groups.push_back(g);
    W.policy.push_back(list[j]);
  }
}


namespace {

// ---- the columns of the pass, their slot-plan chunks and wide groups; rows mode: the column code
//      of every device row (plan->rowcol)
int plan_columns(const Env& E, const Batch& B, const DeviceBatch& D, const int32_t* pols, uint32_t npol,
                 const int32_t* row_policy, int origin, PassPlan* plan) {
  std::vector<int32_t> list;
  std::map<int32_t, uint32_t> col_of;  // rows mode: policy -> column
  if (plan->rows_mode) {
    for (uint64_t r = 0; r < B.n; ++r)
      if (col_of.emplace(row_policy[r], (uint32_t)list.size()).second) list.push_back(row_policy[r]);
  } else {
    list.assign(pols, pols + npol);
  }
  Status st = build_slot_chunks(E, list.data(), (uint32_t)list.size(), origin, plan->rows_mode, &plan->chunks);
  if (!st.ok()) return st.code;
  if (!plan->rows_mode) plan_wide_groups(E, list, nullptr, origin, plan);
  if (plan->rows_mode) {
    std::vector<uint32_t> at(list.size());
    for (uint32_t c = 0; c < plan->chunks.size(); ++c)
      for (uint32_t j = 0; j < plan->chunks[c].ncols; ++j) at[plan->chunks[c].col0 + j] = (c << 16) | j;
    plan_wide_groups(E, list, &at, origin, plan);
    plan->rowcol.resize(B.n);  // (in device-row order)
    for (uint64_t r = 0; r < B.n; ++r) plan->rowcol[r] = at[col_of[row_policy[D.split ? D.perm[r] : r]]];
  }
  plan->nwide = 0;
  plan->wide_policy.clear();
  for (const SlotChunk& c : plan->chunks) {
    const ColInfo* ci = (const ColInfo*)(c.rec.data() + ((const SlotHdr*)c.rec.data())->o_cols);
    for (uint32_t j = 0; j < c.ncols; ++j)
      if (ci[j].wide != ~0u) plan->wide_policy.push_back((int32_t)ci[j].policy);
  }
  plan->nwide = plan->rows_mode ? (plan->wide_policy.empty() ? 0u : 1u) : (uint32_t)plan->wide_policy.size();
  return KW_OK;
}

// ---- what the chunks classify: the string columns read (bits of Str), the families present, the
//      widest chunk's slots, the image and label-value class counts
struct PassNeeds {
  uint32_t need = 0;
  bool any_ctr = false, any_caps = false, any_trs = false, any_lbl = false, any_ctr_fam = false, any_grp = false;
  uint32_t nslots = 1;
  ImgLayout il{0, 0, 0};
  uint32_t nlv = 0;
};

PassNeeds classify_chunks(const std::vector<SlotChunk>& chunks, const DevHeader* H) {
  PassNeeds N;
  for (const SlotChunk& c : chunks) {
    const SlotHdr& h = *(const SlotHdr*)c.rec.data();
    if (h.ns) N.need |= 1u << S_NS;
    if (h.trs) N.need |= 1u << S_IMG, N.any_trs = true;
    if (h.aa) N.need |= 1u << S_AA;
    if (h.caps) N.need |= (1u << S_CAPADD) | (1u << S_CAPDROP), N.any_caps = true;
    if (h.lbl) {
      N.need |= 1u << S_LK;
      if (H->kv_off) N.need |= 1u << S_LV;
      N.any_lbl = true;
    }
    N.any_ctr = N.any_ctr || (h.priv[0] | h.priv[1] | h.priv[2] | h.priv[3] | h.caps | h.aa | h.trs) != 0;
    N.any_ctr_fam = N.any_ctr_fam || (h.priv[0] | h.priv[1] | h.priv[2] | h.priv[3] | h.caps | h.aa) != 0;
    N.any_grp = N.any_grp || c.groups;
    N.nslots = std::max(N.nslots, c.nslots);
  }
  if (H->bypass_cls) N.need |= 1u << S_NS;
  if (N.any_trs) {
    N.il.nreg = (H->col[COL_REG].lit_off ? 1u : 0u) + H->col[COL_REG].ndfa;
    N.il.ntag = (H->col[COL_TAG].lit_off ? 1u : 0u) + H->col[COL_TAG].ndfa;
    N.il.nimg = H->col[COL_IMG].ndfa;
  }
  N.nlv = (N.need & (1u << S_LV)) ? H->col[COL_LV].ndfa : 0u;
  return N;
}

// ---- the classifiers the pass stages (literal tables, DFA chains, the per-key value region) and
//      the launches: chunks grouped so tables + staged records fit the per-workgroup budget; a pass
//      whose tables or a single chunk alone exceed it reads them from global memory (L2)
struct TablePlan {
  struct Stage {
    uint32_t blob, bytes;
  };
  std::vector<Stage> stages;
  uint32_t lit_of[NCOL] = {}, dfa_of[NCOL] = {}, kv_stage = 0;  // index + 1 in stages, 0: not staged
  uint32_t table_bytes = 0;
  bool ldst = false;  // tables and chunk records staged in LDS
  uint32_t area = 0;  // LDS bytes of the largest launch's tables + records (0 when read from global memory)
};

TablePlan plan_tables(const DevHeader* H, uint32_t need, const std::vector<SlotChunk>& chunks,
                      std::vector<std::pair<uint32_t, uint32_t>>* launches) {
  TablePlan P;
  auto stage_col = [&](Col c, bool lit, bool dfa) {
    const DevCol& dc = H->col[c];
    if (lit && dc.lit_off) {
      P.lit_of[c] = (uint32_t)P.stages.size() + 1;
      P.stages.push_back({dc.lit_off, dc.lit_bytes});
    }
    if (dfa && dc.dfa_off) {
      P.dfa_of[c] = (uint32_t)P.stages.size() + 1;
      P.stages.push_back({dc.dfa_off, dc.dfa_bytes});
    }
  };
  if (need & (1u << S_NS)) stage_col(COL_NS, true, false);
  if (need & (1u << S_IMG)) {
    stage_col(COL_REG, true, true);
    stage_col(COL_TAG, true, true);
    stage_col(COL_IMG, false, true);
  }
  if (need & (1u << S_AA)) stage_col(COL_AA, true, false);
  if (need & (1u << S_CAPADD)) stage_col(COL_CAP, true, false);
  if (need & (1u << S_LK)) stage_col(COL_LK, true, false);
  if ((need & (1u << S_LV)) && !PlanKnobs::on<KW_KV_GLOBAL>()) {  // A/B knob
    P.kv_stage = (uint32_t)P.stages.size() + 1;
    P.stages.push_back({H->kv_off, H->kv_bytes});
  }
  for (const TablePlan::Stage& s : P.stages) P.table_bytes += (s.bytes + 15u) & ~15u;

  P.ldst = P.table_bytes <= kTableBudget;
  for (const SlotChunk& c : chunks) P.ldst = P.ldst && P.table_bytes + c.staged <= kTableBudget;
  P.ldst = P.ldst && !PlanKnobs::on<KW_GLOBAL_TABLES>();  // diagnostics / tests
  launches->clear();
  P.area = P.ldst ? P.table_bytes : 0;
  for (uint32_t c = 0; c < chunks.size();) {
    uint32_t e = c, bytes = 0;
    while (e < chunks.size() && e - c < kMaxChunks && (!P.ldst || P.table_bytes + bytes + chunks[e].staged <= kTableBudget))
      bytes += chunks[e++].staged;
    launches->push_back({c, e});
    if (P.ldst) P.area = std::max(P.area, P.table_bytes + bytes);
    c = e;
  }
  return P;
}

constexpr uint32_t align16(uint32_t x) { return (x + 15u) & ~15u; }
uint32_t per_cu(uint32_t lds_bytes) { return std::min<uint32_t>(2048 / kSlotThreads, lds_workgroups_per_cu(lds_bytes)); }

// ---- LDS layout of a tile of `rows` requests after `area` bytes of tables and records, sized for
//      the needs `ts`: the offsets and capacities of a zeroed TileArgs. Capacities shrink until the
//      layout fits the budget (lds_bytes stays above it only when nothing fits).
TileArgs tile_layout(const PassNeeds& N, uint32_t area, uint32_t rows, const TileStats& ts) {
  TileArgs T;
  memset(&T, 0, sizeof(T));
  const uint32_t need = N.need;
  const uint32_t vw_stride = N.nslots | 1u;  // odd stride: lanes (requests) spread over the banks
  const uint32_t nim = N.il.n();
  for (double scale = 1.0;; scale *= 0.8) {
    const uint32_t cmax = std::min<uint32_t>(kMaxTileEntities, (uint32_t)std::max(1.0, scale * ts.ctr));
    const uint32_t kmax = std::min<uint32_t>(kMaxTileEntities, (uint32_t)std::max(1.0, scale * std::max(ts.kadd, ts.kdrop)));
    const uint32_t lmax = std::min<uint32_t>(kMaxTileEntities, (uint32_t)std::max(1.0, scale * ts.lbl));
    uint32_t off = 16 + align16(area);
    auto take = [&](uint32_t bytes) {
      const uint32_t o = off;
      off = align16(off + bytes);
      return o;
    };
    T.o_rf = take(rows);
    T.o_coff = take((rows + 1) * 4);
    T.o_loff = take((rows + 1) * 4);
    T.o_cflags = take(cmax + 8);  // staged from the dword holding the first flag
    T.o_cadd = take((cmax + 1) * 4);
    T.o_cdrop = take((cmax + 1) * 4);
    T.o_ns = take(rows * 2);
    T.o_aa = take((need & (1u << S_AA)) ? cmax * 2 : 0);
    T.o_img = take((need & (1u << S_IMG)) ? cmax * nim * 2 : 0);
    T.o_capadd = take(N.any_caps ? kmax * 2 : 0);
    T.o_capdrop = take(N.any_caps ? kmax * 2 : 0);
    T.o_lk = take(N.any_lbl ? lmax * 2 : 0);
    T.o_lv = take(N.any_lbl ? lmax * N.nlv * 2 : 0);
    T.o_vadd = take(N.any_caps ? kmax * 8 : 0);
    T.o_vl = take(N.any_lbl ? lmax * 8 : 0);
    T.o_vc = take(cmax * 8);
    T.o_vtr = take(N.any_trs ? cmax * 8 : 0);
    T.o_own_c = take(cmax);
    T.o_own_l = take(lmax);
    T.o_rej = take(rows * 8);
    T.o_mut = take(rows * 8);
    T.o_byp = take(rows);
    T.o_sa = take(NSTR * 4);
    T.o_nx = take(16);  // (kernels.hpp TileArgs::o_nx)
    T.o_desc = take(2 * sizeof(TileDesc));
    T.o_pf = l2_prefetch() ? take(4 * kPfLanes) : 0u;
    // union: the staged strings (P0-P1) and the violation words (P2-P3)
    const uint32_t u0 = off;
    uint32_t su = u0;
    for (int m = 0; m < (int)NSTR; ++m) {
      T.o_so[m] = T.o_sb[m] = T.sb_cap[m] = 0;
      if (!(need & (1u << m))) continue;
      const uint32_t cnt = m == S_NS ? rows : (m == S_CAPADD || m == S_CAPDROP) ? kmax : (m == S_LK || m == S_LV) ? lmax : cmax;
      T.o_so[m] = su;
      su = align16(su + (cnt + 1) * 4);
      T.sb_cap[m] = align16((uint32_t)std::min(16384.0, std::max(16.0, scale * ts.bytes[m])));  // longer tiles split
      T.o_sb[m] = su;
      su = align16(su + T.sb_cap[m] + 48);  // slack: batched dword reads may run <= 36 bytes past a string start
    }
    T.o_vw = u0;
    T.vw_stride = vw_stride;
    off = std::max(su, align16(u0 + rows * vw_stride * 4));
    if (off > kTileLdsBudget && scale > 1e-5) continue;  // capacities shrink until the layout fits; bigger tiles split
    T.rows = rows;
    T.cmax = cmax;
    T.kmax = kmax;
    T.lmax = lmax;
    T.lds_bytes = off;
    return T;
  }
}

// What the capacity and tile-height choices of a pass read.
struct TileCtx {
  const Batch& B;
  DeviceBatch& D;  // rows_plans: the batch's tile needs and capacity choices, kept across passes
  const PassNeeds& N;
  uint32_t area;
  bool dump;  // KW_TILE_DEBUG & 256
};

// ---- capacities at a tile height: the highest occupancy (workgroups per CU, LDS-bound) whose layout
// splits at most 2 % of the tiles (a tile beyond the capacities runs as halves, upload_tile_descs),
// over per-dimension quantiles of the tile needs; at a given occupancy the largest capacities
// (fewest split tiles). Chosen once per batch, region [lo, hi), tile height and layout signature.
const DeviceBatch::RowsPlan& plan_rows(const TileCtx& C, uint32_t r, uint64_t lo, uint64_t hi) {
  const PassNeeds& N = C.N;
  const uint64_t key = ((uint64_t)C.area << 40) ^ ((uint64_t)N.nslots << 20) ^ ((uint64_t)N.il.n() << 12) ^ ((uint64_t)N.nlv << 8) ^ N.need;
  DeviceBatch::RowsPlan* R = nullptr;
  for (auto& x : C.D.rows_plans)
    if (x.rows == r && x.lo == lo && x.hi == hi) R = &x;
  if (!R) {
    C.D.rows_plans.emplace_back();
    R = &C.D.rows_plans.back();
    R->rows = r;
    R->lo = lo;
    R->hi = hi;
    R->stride = 0;
  }
  if (R->stride == 0 || R->stride > C.D.needs_stride) {  // (a sampled plan is refined when a pass wants every tile)
    R->stride = std::max<uint32_t>(1, C.D.needs_stride);
    R->need = tile_needs(C.B, r, R->stride, lo, hi);
    R->q = tile_quantiles(R->need, kTileQuantiles, sizeof(kTileQuantiles) / sizeof(kTileQuantiles[0]));
    R->cap_choice = -1;
  }
  if (R->cap_choice < 0 || R->cap_key != key) {
    const uint64_t ntl = R->need.size();
    int best = 0;
    uint32_t best_cu = 0, best_lds = 0;
    const double max_split = PlanKnobs::real<KW_TILE_SPLIT>();  // A/B knob
    for (int k = 0; k < (int)R->q.size(); ++k) {
      const TileArgs T = tile_layout(N, C.area, r, R->q[k]);
      const uint32_t cu = per_cu(T.lds_bytes);
      if (T.lds_bytes > kTileLdsBudget) continue;
      uint64_t over = 0;  // tiles beyond these capacities (split by the descriptors' fit test)
      for (const TileStats& x : R->need) {
        bool o = x.ctr > T.cmax || x.lbl > T.lmax || x.kadd > T.kmax || x.kdrop > T.kmax;
        for (int m = 0; m < (int)NSTR && !o; ++m) o = T.sb_cap[m] && x.bytes[m] > T.sb_cap[m];
        over += o;
      }
      if (C.dump)
        fprintf(stderr, "[kw tile] rows=%u candidate q=%g lds=%u wg/cu=%u split=%llu/%llu\n", r, kTileQuantiles[k], T.lds_bytes, cu,
                (unsigned long long)over, (unsigned long long)ntl);
      if (k > 0 && (double)over > max_split * (double)ntl) continue;
      if (cu > best_cu) {
        best = k;
        best_cu = cu;
        best_lds = T.lds_bytes;
      }
    }
    R->cap_key = key;
    R->cap_choice = best;
    R->cap_cu = best_cu;
    R->cap_lds = best_lds;
  }
  return *R;
}

// ---- tile height of region [lo, hi), with its capacities: KW_SLOT_ROWS when forced; else
// kSlotRows, or a taller tile (128 down to 96 rows)
// when the batch has at least 4 tiles per workgroup slot, the taller layout still keeps 4
// workgroups per CU (its LDS estimated from the 64-row layout first: the per-request part scales
// with the height), and at most KW_ROUND_SPLIT (2 %) of its tiles hold more items in one P1
// segment (labels, capability strings, containers / images) than the workgroup has lanes: such a
// tile sends one wave through the segment twice, and its phase waits for that wave (r03: half of
// C2 / C3's 128-row tiles had more than 256 images). Taller tiles amortise the per-tile latency
// (staging, barriers) where the per-request LDS is small: C2 -12 %, C3 -25 % at 128 rows (r02);
// the C4-C6 layouts need 64 rows for 4 workgroups per CU (r02 sweeps). Per region: a split
// batch's light region takes the capacities (and occupancy) of its own tiles.
const DeviceBatch::RowsPlan& pick_rows(const TileCtx& C, uint64_t lo, uint64_t hi) {
  if (const uint32_t f = slot_rows_forced()) return plan_rows(C, f, lo, hi);
  if (lo > 0) {
    // the heavy region of a split batch: the tallest tile height whose capacities reach the
    // kernel's register-bound occupancy (<= 128 VGPRs: 4 workgroups of 256 threads per CU), else
    // the one with the most workgroups per CU. r05 C5 sweep (profiles/r05_split_ab.txt): at equal
    // occupancy taller tiles win (heavy > 5: 12 rows 6.31 ms, 10 rows 6.85), and a layout one
    // workgroup per CU short loses 10-15 % whatever its height.
    if (const uint32_t h = heavy_rows()) return plan_rows(C, h, lo, hi);
    const DeviceBatch::RowsPlan* pick = nullptr;
    for (uint32_t r : {64u, 48u, 40u, 32u, 28u, 24u, 20u, 16u, 14u, 12u, 10u, 8u}) {
      const DeviceBatch::RowsPlan& R = plan_rows(C, r, lo, hi);
      if (!pick || R.cap_cu > pick->cap_cu) pick = &R;
      if (R.cap_cu >= 4) break;
    }
    return *pick;
  }
  const PassNeeds& N = C.N;
  const double round_split = PlanKnobs::real<KW_ROUND_SPLIT>();  // A/B knob
  auto two_rounds = [&](const DeviceBatch::RowsPlan& R) {  // share of tiles with a segment beyond one round
    uint64_t over = 0;
    for (const TileStats& x : R.need) {
      uint32_t seg = 0;
      if (N.any_lbl) seg = std::max(seg, x.lbl);
      if (N.any_caps) seg = std::max(seg, x.kadd + x.kdrop);
      if (N.any_ctr || (N.need & (1u << S_IMG))) seg = std::max(seg, x.ctr);
      over += seg > kSlotThreads;
    }
    return R.need.empty() ? 0.0 : (double)over / (double)R.need.size();
  };
  const DeviceBatch::RowsPlan& base = plan_rows(C, kSlotRows, lo, hi);
  const uint32_t fixed = 16 + align16(C.area), per64 = base.cap_lds > fixed ? base.cap_lds - fixed : 0u;
  for (uint32_t r : {128u, 120u, 112u, 104u, 96u}) {
    const uint64_t est = fixed + (uint64_t)per64 * r / kSlotRows;
    if (C.dump)
      fprintf(stderr, "[kw tile] rows=%u estimated lds=%llu (64-row layout %u, fixed %u) region rows %llu\n", r,
              (unsigned long long)est, base.cap_lds, fixed, (unsigned long long)(hi - lo));
    if (per_cu((uint32_t)std::min<uint64_t>(est, 1u << 30)) < 4 || hi - lo < (uint64_t)r * 4 * 256 * 4) continue;
    const DeviceBatch::RowsPlan& R = plan_rows(C, r, lo, hi);
    const double tr = two_rounds(R);
    if (C.dump)
      fprintf(stderr, "[kw tile] rows=%u workgroups/CU %u, tiles with a segment beyond %u items %.4f\n", r, R.cap_cu,
              kSlotThreads, tr);
    if (R.cap_cu >= 4 && tr <= round_split) return R;
  }
  return base;
}

// ---- one region's geometry: the layout at the picked height and capacities, its grid and schedule.
// False when the policy list is too large for one tile.
bool plan_region(const TileCtx& C, const DeviceBatch::RowsPlan& pick, bool ldst, PassPlan::Region* g) {
  TileArgs& T = g->geom;
  if (PlanKnobs::is_set<KW_TILE_QUANTILE>())  // tests / diagnostics: force the capacity quantile
    T = tile_layout(C.N, C.area, pick.rows, tile_quantile(pick.need, PlanKnobs::real<KW_TILE_QUANTILE>()));
  else
    T = tile_layout(C.N, C.area, pick.rows, pick.q[pick.cap_choice]);
  if (T.lds_bytes > kTileLdsBudget) return false;
  // next-tile L2 prefetch (compiled in with KW_PREFETCH, kernels.hpp): a gain where several small
  // tiles share a CU, a loss where two large ones do (C5: +2.7 %; r02 A/B); off by default since the
  // descriptor moved to LDS (r02 s60)
  T.prefetch = l2_prefetch() && per_cu(T.lds_bytes) >= 3 ? 1u : 0u;
  // predecessor ranges four loads a round where tiles hold many containers per request (C5 -6 %;
  // C4, two per request, keeps the plain loops: r02 s80)
  T.ctr_ranges = T.cmax > 4u * T.rows ? 1u : 0u;
  g->lo = pick.lo;
  g->hi = pick.hi;
  const uint64_t nt = (g->hi - g->lo + T.rows - 1) / T.rows;
  g->grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nt, 256ull * per_cu(T.lds_bytes)));
  g->dyn = sched_dynamic(nt, g->grid, ldst);
  return true;
}

// ---- the fields every region shares
void share_fields(TileArgs& T, const DevHeader* H, const PassNeeds& N, const TablePlan& P, const DeviceBatch& D,
                  bool rows_mode, uint32_t debug) {
  const uint32_t need = N.need;
  const bool ldst = P.ldst;
  T.feat = ((need & (1u << S_IMG)) ? kFeatImg : 0u) | (N.any_lbl ? kFeatLbl : 0u) | (N.any_ctr_fam ? kFeatCtr : 0u) |
           (N.any_grp ? kFeatGrp : 0u);
  // NFA elements among the classifiers the pass reads: the one instantiation that reads their classes
  const bool nfa_img = (need & (1u << S_IMG)) &&
                       ((H->col[COL_REG].flags | H->col[COL_TAG].flags | H->col[COL_IMG].flags) & 1u);
  const bool nfa_lv = (need & (1u << S_LV)) && (H->col[COL_LV].flags & 1u);
  if (nfa_img || nfa_lv) T.feat = kFeatAll | kFeatNfa;
  // many containers per request (C5's heavy region): the wave-scan instantiation (kernels.hpp kFeatRng)
  if (T.ctr_ranges && ldst && T.feat == (kFeatLbl | kFeatCtr)) T.feat |= kFeatRng;
  T.il = N.il;
  T.nlv = N.nlv;
  T.need = need;
  T.lds_tables = ldst ? 1u : 0u;
  T.nlk = H->col[COL_LK].nclass;
  T.bypass_cls = H->bypass_cls;
  T.docker_io_cls = H->docker_io_cls;
  T.latest_cls = H->latest_cls;
  T.rows_mode = rows_mode ? 1u : 0u;
  for (int m = 0; m < (int)NSTR; ++m) {
    T.s_off[m] = D.str[m].off;
    T.s_bytes[m] = D.str[m].bytes;
  }
  // classifiers: blob offsets, and their LDS positions when staged
  const auto& stages = P.stages;
  uint32_t at = 16;
  std::vector<uint32_t> lds_at(stages.size());
  for (size_t k = 0; k < stages.size(); ++k) {
    lds_at[k] = at;
    at += (stages[k].bytes + 15u) & ~15u;
  }
  T.nstage = 0;
  if (ldst)
    for (size_t k = 0; k < stages.size(); ++k) {
      T.stage_blob[T.nstage] = stages[k].blob;
      T.stage_lds[T.nstage] = lds_at[k];
      T.stage_bytes[T.nstage] = (stages[k].bytes + 15u) & ~15u;
      ++T.nstage;
    }
  for (int c = 0; c < (int)NCOL; ++c) {
    if (P.lit_of[c]) {
      T.lit_blob[c] = stages[P.lit_of[c] - 1].blob;
      T.lit_lds[c] = lds_at[P.lit_of[c] - 1];
    }
    if (P.dfa_of[c]) {
      T.dfa_blob[c] = stages[P.dfa_of[c] - 1].blob;
      T.dfa_lds[c] = lds_at[P.dfa_of[c] - 1];
    }
  }
  if (P.kv_stage) {
    T.kv_blob = stages[P.kv_stage - 1].blob;
    T.kv_lds = ldst ? lds_at[P.kv_stage - 1] : 0u;
  } else if (need & (1u << S_LV)) {  // the value DFAs read from the blob (global memory, L1/L2)
    T.kv_blob = H->kv_off;
    T.kv_lds = 0;
  }
  T.debug = debug;  // phase ablation (diagnostics)
  T.generic = PlanKnobs::on<KW_TILE_GENERIC>() ? 1u : 0u;  // (kernels.hpp tile_prod_shape)
  const void* const cols[6] = {D.req_flags, D.ctr_off, D.lbl_off, D.ctr_flags, D.capadd_off, D.capdrop_off};
  build_copy_jobs(&T, cols);
}

// KW_TILE_DEBUG & 256: a region's plan on stderr (scripts/diag.sh reads these lines).
void dump_plan(const TileArgs& T, const PassNeeds& N, const TablePlan& P, size_t nchunks, size_t nlaunches) {
  fprintf(stderr, "[kw tile] lds_tables=%u rows=%u cmax=%u kmax=%u lmax=%u lds=%u area=%u (classifiers %u) chunks=%zu launches=%zu nim=%u nlv=%u\n",
          T.lds_tables, T.rows, T.cmax, T.kmax, T.lmax, T.lds_bytes, P.area, P.table_bytes, nchunks, nlaunches, N.il.n(), N.nlv);
  for (size_t k = 0; k < P.stages.size(); ++k) fprintf(stderr, "[kw tile]   classifier stage %zu: %u bytes\n", k, P.stages[k].bytes);
  // the tile's LDS regions (bytes): per-request state, entity classes and sets, the strings / violation-words union
  uint32_t so = 0, sb = 0;
  for (int m = 0; m < (int)NSTR; ++m)
    if (T.o_sb[m]) so += T.o_sb[m] - T.o_so[m], sb += T.sb_cap[m] + 48;
  fprintf(stderr,
          "[kw tile]   layout: headers %u | classes ns %u aa %u img %u caps %u lk %u lv %u | sets vadd %u vl %u vc %u vtr %u | "
          "owners %u | rej/mut/byp %u | union at %u: string offsets %u + bytes %u, violation words %u | total %u\n",
          T.o_ns - T.o_rf, T.o_aa - T.o_ns, T.o_img - T.o_aa, T.o_capadd - T.o_img, T.o_lk - T.o_capadd, T.o_lv - T.o_lk,
          T.o_vadd - T.o_lv, T.o_vl - T.o_vadd, T.o_vc - T.o_vl, T.o_vtr - T.o_vc, T.o_own_c - T.o_vtr, T.o_rej - T.o_own_c,
          T.o_sa - T.o_rej, T.o_vw, so, sb, T.rows * T.vw_stride * 4, T.lds_bytes);
}

// ---- per-launch TileArgs (record pointers filled in at upload, run_pass), region by region
void plan_launch_args(const TablePlan& P, uint32_t npol, PassPlan* plan) {
  plan->slot_blob.clear();
  plan->slot_at.clear();
  for (const SlotChunk& c : plan->chunks) {
    plan->slot_at.push_back((uint32_t)plan->slot_blob.size());
    plan->slot_blob.insert(plan->slot_blob.end(), c.rec.begin(), c.rec.end());
  }
  plan->tiles.clear();
  for (const PassPlan::Region& rg : plan->regions)
    for (const auto& [c0, c1] : plan->launches) {
      TileArgs t = rg.geom;
      t.nchunk = c1 - c0;
      uint32_t at = 16 + P.table_bytes;
      for (uint32_t k = 0; k < t.nchunk; ++k) {
        const SlotChunk& c = plan->chunks[c0 + k];
        ChunkArgs& ca = t.chunk[k];
        memset(&ca, 0, sizeof(ca));
        ca.o_lds = P.ldst ? at : 0u;
        at += c.staged;
        ca.col0 = c.col0;
        ca.ncols = c.ncols;
        ca.vec4 = (!plan->rows_mode && npol % 4u == 0 && c.col0 % 4u == 0 && c.ncols % 4u == 0) ? 1u : 0u;
        ca.init = ((const SlotHdr*)c.rec.data())->init;
      }
      plan->tiles.push_back(t);
    }
}

// ---- evaluation arguments and the pass's algorithmic bytes; KW_E_ARG when a column the kernel
//      dereferences is missing (a null column is a device fault)
int plan_eval_args(const Env& E, const Batch& B, const DeviceBatch& D, const PassNeeds& N, uint32_t npol, int origin,
                   PassPlan* plan) {
  EvalArgs& A = plan->args;
  memset(&A, 0, sizeof(A));
  A.blob = (const uint8_t*)E.d_blob;
  A.nrows = B.n;
  A.npol = plan->rows_mode ? 1u : npol;
  A.origin = origin;
  A.req_flags = D.req_flags;
  A.ctr_off = D.ctr_off;
  A.lbl_off = D.lbl_off;
  A.ctr_flags = D.ctr_flags;
  A.capadd_off = D.capadd_off;
  A.capdrop_off = D.capdrop_off;
  A.out = D.verdicts;
  A.nwide = plan->nwide;
  plan->wide_cap_per_row = plan->rows_mode ? 1u : npol;
  if (!A.req_flags || !A.ctr_off || !A.lbl_off || !A.ctr_flags || !A.capadd_off || !A.capdrop_off || !A.out) return KW_E_ARG;
  for (int m = 0; m < (int)NSTR; ++m)
    if ((N.need & (1u << m)) && (!plan->geom.s_off[m] || !plan->geom.s_bytes[m])) return KW_E_ARG;

  // algorithmic bytes: request headers once, the entity columns and strings the policies read, and
  // the verdict words written
  const double n = (double)B.n;
  double eb = n * (1 + 4 + 4) + 4.0 * n * (double)A.npol;
  if (N.any_ctr) eb += (double)B.containers() * 1.0;
  if (N.any_caps) eb += (double)B.containers() * 8.0;
  for (int m = 0; m < (int)NSTR; ++m)
    if (N.need & (1u << m)) eb += (double)D.str[m].nbytes + 4.0 * (double)D.str[m].n;
  plan->evaluate_bytes = eb;
  return KW_OK;
}

}  // namespace

// ---- P0's copy-job table (kernels.hpp CopyJob) from a TileArgs whose LDS layout and string
// columns are set. Descriptor words by their position in TileDesc.
void build_copy_jobs(TileArgs* Tp, const void* const cols[6]) {
  TileArgs& T = *Tp;
  constexpr uint32_t W_CB = offsetof(TileDesc, cb) / 4, W_CE = offsetof(TileDesc, ce) / 4, W_LB = offsetof(TileDesc, lb) / 4,
                     W_LE = offsetof(TileDesc, le) / 4, W_KAB = offsetof(TileDesc, kab) / 4, W_KAE = offsetof(TileDesc, kae) / 4,
                     W_KDB = offsetof(TileDesc, kdb) / 4, W_KDE = offsetof(TileDesc, kde) / 4, W_SA = offsetof(TileDesc, sa) / 4,
                     W_NV = offsetof(TileDesc, nv) / 4, W_R0 = offsetof(TileDesc, r0lo) / 4, W_NR = offsetof(TileDesc, nr) / 4;
  static_assert(W_NR < 32 && offsetof(TileDesc, r0hi) / 4 == W_R0 + 1, "copy_code holds 5-bit descriptor words");
  struct Todo {
    CopyJob j;
    uint32_t trips;  // copy instructions a wave issues for a tile at the layout's capacities
  };
  std::vector<Todo> todo;
  auto add = [&](const void* base, uint32_t code, uint32_t pieces) {
    todo.push_back({{(uint64_t)(uintptr_t)base, code, 0u}, (pieces + 63u) / 64u});
  };
  const uint32_t req = kCjRel | kCjReq, offs = kCjElem4 | kCjPlus1;  // request-indexed; an offsets array
  add(cols[0], copy_code(W_R0, W_NR, T.o_rf, req | kCjQuad), (T.rows + 3) / 4);
  add(cols[1], copy_code(W_R0, W_NR, T.o_coff, req | offs), T.rows + 1);
  add(cols[2], copy_code(W_R0, W_NR, T.o_loff, req | offs), T.rows + 1);
  add(cols[3], copy_code(W_CB, W_CE, T.o_cflags, kCjQuad | kCjAlign), (T.cmax + 3) / 4 + 1);
  add(cols[4], copy_code(W_CB, W_CE, T.o_cadd, offs), T.cmax + 1);
  add(cols[5], copy_code(W_CB, W_CE, T.o_cdrop, offs), T.cmax + 1);
  for (uint32_t m = 0; m < NSTR; ++m) {
    if (!T.o_sb[m]) continue;
    uint32_t wb = W_CB, we = W_CE, fl = offs, cap = T.cmax;
    if (m == S_NS) wb = W_R0, we = W_NR, fl |= req, cap = T.rows;
    else if (m == S_CAPADD) wb = W_KAB, we = W_KAE, cap = T.kmax;
    else if (m == S_CAPDROP) wb = W_KDB, we = W_KDE, cap = T.kmax;
    else if (m == S_LK || m == S_LV) wb = W_LB, we = W_LE, cap = T.lmax;
    add(T.s_off[m], copy_code(wb, we, T.o_so[m], fl), cap + 1);
    add(T.s_bytes[m], copy_code(W_SA + m, W_NV + m, T.o_sb[m], kCjRel | kCjX4), T.sb_cap[m] / 16);
  }
  // job j runs on wave j % 4: the longest jobs first, dealt to the waves back and forth, so each
  // wave's copy instructions come out about even
  std::stable_sort(todo.begin(), todo.end(), [](const Todo& a, const Todo& b) { return a.trips > b.trips; });
  memset(T.jobs, 0, sizeof(T.jobs));
  T.njobs = (uint32_t)todo.size();
  for (uint32_t k = 0; k < T.njobs; ++k) {
    const uint32_t row = k / 4u, i = k % 4u;
    const uint32_t len = std::min(4u, T.njobs - row * 4u);  // (the last row may be short)
    T.jobs[row * 4u + ((row & 1u) ? len - 1u - i : i)] = todo[k].j;
  }
}

// Plan one pass: slot-plan chunks of the policy list, the launches they take, the tile geometry
// and LDS layout, the kernel arguments.
int plan_pass(const kw_env* env, kw_batch* kb, const int32_t* pols, uint32_t npol, const int32_t* row_policy,
              int origin, bool timing, PassPlan* plan) {
  const Env& E = env->e;
  DeviceBatch& D = *kb->dev;
  const Batch& B = dev_rows(kb);
  const DevHeader* H = (const DevHeader*)E.blob.data();
  plan->env_blob = E.blob.data();
  plan->rows_mode = row_policy != nullptr;
  const uint32_t debug = (uint32_t)PlanKnobs::num<KW_TILE_DEBUG>();
  const auto pt0 = std::chrono::steady_clock::now();
  auto pms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pt0).count(); };

  if (int rc = plan_columns(E, B, D, pols, npol, row_policy, origin, plan)) return rc;
  const double t_slots = timing ? pms() : 0.0;
  const PassNeeds N = classify_chunks(plan->chunks, H);
  const TablePlan P = plan_tables(H, N.need, plan->chunks, &plan->launches);

  // tile geometry per region: one, or the light and heavy regions of a split batch
  const TileCtx C{B, D, N, P.area, (debug & 256u) != 0};
  std::vector<std::pair<uint64_t, uint64_t>> bounds{{0, B.n}};
  if (D.split && D.split < B.n) bounds = {{0, D.split}, {D.split, B.n}};
  plan->regions.clear();
  for (const auto& [lo, hi] : bounds) {
    const DeviceBatch::RowsPlan& pick = pick_rows(C, lo, hi);
    if (timing) fprintf(stderr, "[kw plan] slot chunks %.2f ms, tile needs + capacities %.2f ms\n", t_slots, pms() - t_slots);
    PassPlan::Region g;
    if (!plan_region(C, pick, P.ldst, &g)) return KW_E_ARG;  // policy list too large for one tile
    plan->regions.push_back(g);
  }
  for (PassPlan::Region& rg : plan->regions) {
    share_fields(rg.geom, H, N, P, D, plan->rows_mode, debug);
    if (C.dump) dump_plan(rg.geom, N, P, plan->chunks.size(), plan->launches.size());
  }
  plan->geom = plan->regions[0].geom;
  plan->grid = plan->regions[0].grid;

  plan_launch_args(P, npol, plan);
  return plan_eval_args(E, B, D, N, npol, origin, plan);
}

}  // namespace kw
