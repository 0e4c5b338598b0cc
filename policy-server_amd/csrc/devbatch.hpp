// devbatch.hpp — the handles behind include/kwgpu.h (kw_env, kw_batch), the device copy of a batch
// (DeviceBatch) and the plan of one pass over it (PassPlan; plan.cpp fills it, pass.cpp runs it).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <deque>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/kwgpu.h"
#include "batch.hpp"
#include "digest.hpp"
#include "env.hpp"
#include "groups.hpp"
#include "kernels.hpp"
#include "pools.hpp"
#include "slotplan.hpp"

struct kw_env {
  kw::Env e;
  // identity of this environment for plan caches (an address can be reused by a later one)
  uint64_t uid = next_uid();
  static uint64_t next_uid() {
    static std::atomic<uint64_t> n{1};
    return n++;
  }
};

namespace kw {

// Per-tile entity counts and staged byte ranges of a batch, reduced to a high quantile (tile_quantile).
struct TileStats {
  uint32_t ctr = 0, lbl = 0, kadd = 0, kdrop = 0;
  uint32_t bytes[NSTR] = {};
};

// A split batch's entity maps (upload_batch, permute_batch): the source entity of each destination
// entity, per level — what the upload gathers the string bytes by (gather_column).
struct RowOrder {
  const std::vector<uint64_t>* perm = nullptr;  // rows (DeviceBatch::perm)
  std::vector<uint32_t> cmap, lmap, amap, dmap;  // containers, labels, added / dropped capabilities
  uint64_t src(int m, uint64_t e) const {
    switch (m) {
      case S_NS: return (*perm)[e];
      case S_CAPADD: return amap[e];
      case S_CAPDROP: return dmap[e];
      case S_LK: case S_LV: return lmap[e];
      default: return cmap[e];
    }
  }
};

struct PassPlan {
  bool rows_mode = false;
  const uint8_t* env_blob = nullptr;  // host copy of the environment's blob (DevHeader first)
  NfaPass nfa{};                      // filled by ensure_nfa when the pass has NFA elements
  uint32_t nfa_threads = 0;
  std::vector<SlotChunk> chunks;
  std::vector<std::pair<uint32_t, uint32_t>> launches;  // chunk ranges [first, last)
  std::vector<TileArgs> tiles;                          // one per launch (record pointers filled at upload)
  std::vector<uint8_t> slot_blob;                       // the chunks' records, concatenated
  std::vector<uint32_t> slot_at;                        // offset of each chunk's record in slot_blob
  TileArgs geom;  // the first region's geometry (the fields every region shares)
  EvalArgs args;
  uint32_t grid = 0;
  // tile geometry per region of the device rows: one, or the light and heavy regions of a split
  // batch (DeviceBatch::split), each with its own capacities, LDS layout and grid; `tiles` holds
  // region k's launches at [k * launches.size(), (k + 1) * launches.size())
  struct Region {
    uint64_t lo = 0, hi = 0;
    TileArgs geom;
    uint32_t grid = 0;
    bool dyn = true;  // the dynamic tile schedule (sched_dynamic), else the strided one
  };
  std::vector<Region> regions;
  uint32_t nwide = 0;
  std::vector<int32_t> wide_policy;
  std::vector<uint32_t> rowcol;  // rows mode
  uint64_t wide_cap_per_row = 0;
  double evaluate_bytes = 0;
  // wide policy groups of the pass (> 64 members or deep stacks): their combine records, jump
  // code, member slot -> member-pass column maps, the member-pass policy list
  struct Wide {
    std::vector<WideGroupArgs> groups;
    std::vector<int32_t> policy;
    std::vector<uint8_t> progs;
    std::vector<uint32_t> midx;
    std::vector<int32_t> members;
    // split group members (env.cpp split_policy): records of kind 2 / 3 after the groups' own in
    // the upload; a member slot's midx entry is kSplitMember | record index
    std::vector<WideGroupArgs> aux;
    uint32_t cause_stride = 0, stack_words = 0;
  } wide;
};

// Device copy of a batch: one allocation for the input columns, lazily sized verdict / plan /
// side-data buffers, a private stream and timing events.
struct DeviceBatch {
  int device = -1;
  hipStream_t stream = nullptr;  // the batch's stream (passes without a caller stream)
  bool owns_stream = true;       // false: the caller's stream (kw_batch_to_device_async)
  void* staging = nullptr;       // pinned host staging of the last upload
  size_t staging_bytes = 0;
  hipStream_t cur = nullptr;     // stream of the last pass (kw_batch_verdicts synchronises on it)
  uint8_t* cols = nullptr;
  size_t cols_bytes = 0;
  // device views of the columns
  const uint8_t* req_flags = nullptr;
  const uint32_t *ctr_off = nullptr, *lbl_off = nullptr, *capadd_off = nullptr, *capdrop_off = nullptr;
  const uint8_t* ctr_flags = nullptr;
  struct DCol {
    const uint32_t* off = nullptr;
    const uint8_t* bytes = nullptr;
    uint64_t n = 0;
    uint64_t nbytes = 0;
  } str[NSTR];
  uint32_t* verdicts = nullptr;
  size_t verdict_cap = 0;
  size_t last_verdicts = 0;
  uint32_t last_row_words = 0;  // verdict words per row of the last pass (npol; rows mode 1)
  // light / heavy split (upload_batch, split_rows): the device copy holds the batch's rows in
  // another order — the light rows, then the heavy ones — and every device buffer indexed by row
  // (verdicts, side data, the rows-mode column map) follows that order; kw_batch_verdicts and
  // load_side_data scatter them back. perm[d]: the batch row at device row d; split: the light
  // region's rows (0: not split); dev_b: the reordered batch the planner reads (its offsets only:
  // the string bytes are dropped after the upload).
  std::vector<uint64_t> perm;
  std::vector<uint64_t> inv_perm;  // the device row of each batch row (device_rows builds it once)
  uint64_t split = 0;
  // The device row of each batch row of a split batch, for the entries that take batch rows and
  // index device buffers (kw_batch_verdict_rows, kw_batch_outcomes).
  const std::vector<uint64_t>& device_rows() {
    if (inv_perm.size() != perm.size()) {
      inv_perm.resize(perm.size());
      for (uint64_t d = 0; d < perm.size(); ++d) inv_perm[perm[d]] = d;
    }
    return inv_perm;
  }
  std::unique_ptr<Batch> dev_b;
  // the last all-pairs pass's plan (pass.cpp validate_cached): reused while the
  // environment, the policy list, the origin and every KW_* setting stay the same — planning a
  // 64-policy pass is ~60-300 us of host time, the whole GPU time of a small shard
  std::shared_ptr<PassPlan> plan_cache;
  uint64_t plan_env = 0, plan_knobs = 0;
  std::vector<int32_t> plan_pols;
  int plan_origin = -1;
  std::unique_ptr<RowOrder> order;  // (until the upload's staging is filled)
  uint32_t loaded = 0;        // string columns (bits of Str) whose bytes are resident (kw_validate_host uploads only its pass's)
  uint32_t* sched = nullptr;  // tile counters (zeroed once; each launch leaves them zero)
  std::vector<int64_t> last_launches;  // the last pass's tile launches: (workgroups launched, descriptors, static rounds or -1) each (diagnostic)
  std::vector<uint32_t> last_kernels;  // the kernel each of those launches took (kernels.hpp tile_kernel_kind)
  std::vector<uint32_t> last_variants;  // and the variant each asked the dispatch for (kernels.hpp tile_variant_word)
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  // the last pass's plan as the kernels read it (host copies detect a changed plan)
  TileArgs* d_tiles = nullptr;
  size_t d_tiles_cap = 0;
  std::vector<TileArgs> h_tiles;
  uint8_t* d_slots = nullptr;
  size_t d_slots_cap = 0;
  std::vector<uint8_t> h_slots;
  uint32_t* rowcol = nullptr;
  size_t rowcol_cap = 0;
  std::vector<uint32_t> h_rowcol;
  // host-built tile descriptors + overflow list, cached for one plan geometry (desc_key)
  TileDesc* desc = nullptr;
  size_t desc_cap = 0;
  uint32_t* overflow = nullptr;  // [count, request indices...]
  size_t overflow_cap = 0;
  std::vector<TileDesc> h_desc;
  std::vector<uint32_t> h_ovf;
  uint32_t n_overflow = 0;
  uint64_t ndesc = 0;
  uint64_t reg_desc[2] = {0, 0}, reg_ndesc[2] = {0, 0};  // each region's descriptors within desc
  uint64_t desc_key = 0;
  bool desc_valid = false;   // D.desc holds the whole batch's descriptors for desc_key
  uint32_t needs_stride = 1;  // tile needs sampled every needs_stride-th tile (set by kw_validate_host)
  // overflow path: per-string classes in HBM (one allocation) and the wide-argument side data
  uint16_t* g_cls = nullptr;
  size_t g_cls_cap = 0;
  // NFA elements: their classes ([label][nlv] | [container][nim]) and the Pike VMs' scratch
  uint16_t* nfa_cls = nullptr;
  size_t nfa_cls_cap = 0;
  uint32_t* nfa_scratch = nullptr;
  size_t nfa_scratch_cap = 0;
  uint32_t max_image_len = 0xffffffffu;  // longest image reference of the batch (computed on first use)
  uint32_t* wide_count = nullptr;
  bool wide_valid = false;  // the last pass zeroed wide_count and ran the overflow kernels
  WideRec* wide_rec = nullptr;
  size_t wide_rec_cap = 0;
  uint64_t* wide_groups = nullptr;
  size_t wide_groups_cap = 0;
  // wide policy groups (WideGroupPass): the members' pass output, the combine kernel's records,
  // value-stack scratch and the cause bitsets
  uint32_t* member_words = nullptr;
  size_t member_words_cap = 0;
  uint8_t* wg_data = nullptr;
  size_t wg_data_cap = 0;
  uint64_t* wg_stack = nullptr;
  size_t wg_stack_cap = 0;
  uint64_t* big_causes = nullptr;
  size_t big_causes_cap = 0;
  uint32_t last_big_stride = 0;
  std::vector<WideData::BigRef> last_big_ref;
  // what the last pass left in the side buffers
  uint32_t last_nwide = 0, last_wide_cap = 0;
  bool last_rows_mode = false;
  std::vector<int32_t> last_wide_policy;
  // the last kw_batch_digest (kw_debug_digest_stats): ranges run, leftovers, table slots, ranges cut
  bool digest_ran = false;
  uint64_t digest_stats[4] = {0, 0, 0, 0};
  // the container names (kw_batch_messages uploads them on first use: no pass reads them), in the
  // device's container order: one block [offsets | bytes and their zero tail], kept while this
  // device copy lives
  uint8_t* names = nullptr;
  size_t names_bytes = 0;
  DCol name_col;
  // the last kw_batch_messages (kw_debug_messages_stats): rounds, windows written, messages that
  // spanned a window, items left to the host, whether it uploaded the names
  bool messages_ran = false;
  uint64_t messages_stats[5] = {0, 0, 0, 0, 0};
  // the uid column (kw_batch_responses uploads it on first use, as the names are), in device-row
  // order: one block [offsets | bytes and their zero tail]
  uint8_t* uids = nullptr;
  size_t uids_bytes = 0;
  DCol uid_col;
  // the last kw_batch_responses (kw_debug_responses_stats): rounds, windows written, responses that
  // spanned a window, items left to the host, whether it uploaded a side column, pieces that grew by
  // escaping
  bool responses_ran = false;
  uint64_t responses_stats[6] = {0, 0, 0, 0, 0, 0};
  // the patch-shape columns (kw_batch_patches uploads them on first use, as the uids are; dropped
  // by kw_batch_set_patch_shape), in the device's container and row order: one block
  // [u32 per container | u8 per row]
  uint8_t* places = nullptr;
  size_t places_bytes = 0;
  const uint32_t* ctr_place = nullptr;
  const uint8_t* req_place = nullptr;
  // the last kw_batch_patches (kw_debug_patches_stats): rounds, windows written, items that spanned
  // a window, items left to the host, whether it uploaded a side column (the last is unused)
  bool patches_ran = false;
  uint64_t patches_stats[6] = {0, 0, 0, 0, 0, 0};
  // tile capacities of this batch (plan_pass), per tile height tried
  struct RowsPlan {
    uint32_t rows = 0;
    uint64_t lo = 0, hi = 0;         // the region's rows
    uint32_t stride = 1;            // needs of every stride-th tile (kw_validate_host samples)
    std::vector<TileStats> need, q;  // per-tile needs and their quantiles
    uint64_t cap_key = 0;
    int cap_choice = -1;   // quantile index chosen for cap_key
    uint32_t cap_cu = 0;   // its workgroups per CU
    uint32_t cap_lds = 0;  // its LDS bytes
  };
  std::deque<RowsPlan> rows_plans;  // deque: plan_rows hands out references that must survive later insertions
  ~DeviceBatch() {
    if (device < 0) return;  // host-only view (kw_debug_plan)
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (cur && cur != stream) (void)hipStreamSynchronize(cur);
    BlockPool& P = dev_pool();
    P.release(device, d_tiles, d_tiles_cap * sizeof(TileArgs));
    P.release(device, d_slots, d_slots_cap);
    P.release(device, rowcol, rowcol_cap * 4);
    P.release(device, desc, desc_cap * sizeof(TileDesc));
    P.release(device, overflow, overflow_cap * 4);
    P.release(device, cols, cols_bytes);
    P.release(device, names, names_bytes);
    P.release(device, uids, uids_bytes);
    P.release(device, places, places_bytes);
    P.release(device, verdicts, verdict_cap * 4);
    P.release(device, g_cls, g_cls_cap * 2);
    P.release(device, nfa_cls, nfa_cls_cap * 2);
    P.release(device, nfa_scratch, nfa_scratch_cap * 4);
    P.release(device, wide_rec, wide_rec_cap * sizeof(WideRec));
    P.release(device, wide_groups, wide_groups_cap * 8);
    P.release(device, member_words, member_words_cap * 4);
    P.release(device, wg_data, wg_data_cap);
    P.release(device, wg_stack, wg_stack_cap * 8);
    P.release(device, big_causes, big_causes_cap * 8);
    P.release(device, sched, 512 * sizeof(uint32_t));  // every launch leaves the tile counters zero
    P.release(device, wide_count, sizeof(uint32_t));
    host_pool().release(device, staging, staging_bytes);
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    if (stream && owns_stream) stream_pool().put(device, stream);
  }
};

}  // namespace kw

struct kw_batch {
  kw::Batch b;
  std::unique_ptr<kw::DeviceBatch> dev;
  std::vector<void*> host_pinned;  // kw_batch_pin_host: column arrays page-locked in place
  // kw_batch_attribute_groups: the dictionary of the rows' metrics attributes, built once (the
  // columns of a batch do not change after it is made)
  struct AttrGroups {
    std::mutex m;
    bool built = false;
    std::vector<uint32_t> row_group;
    std::vector<uint64_t> first_row;
  };
  mutable AttrGroups attr;
  ~kw_batch() {
    dev.reset();  // synchronizes the batch's streams: no copy can still read a registered column
    for (void* p : host_pinned) (void)hipHostUnregister(p);
  }
};

namespace kw {

inline const StrCol& host_str(const Batch& B, int m) {
  switch (m) {
    case S_NS: return B.ns;
    case S_IMG: return B.ctr_image;
    case S_AA: return B.ctr_aa;
    case S_CAPADD: return B.cap_add;
    case S_CAPDROP: return B.cap_drop;
    case S_LK: return B.lbl_key;
    default: return B.lbl_val;
  }
}

// The rows the device holds, in device order: the reordered copy of a split batch, else the batch.
inline const Batch& dev_rows(const kw_batch* kb) { return kb->dev && kb->dev->dev_b ? *kb->dev->dev_b : kb->b; }

// The columns a finding's key is cut from (digest.hpp digest_key; digest.cpp): the host batch's, in
// batch rows, and the device copy's, in device rows, where a string column that is not resident
// stays absent.
DigestCols host_cols(const Batch& B);
DigestCols device_cols(const kw_batch* kb);

}  // namespace kw
