// pass.hpp — running a planned pass (plan.cpp) on a resident batch and reading its results back
// (pass.cpp): the plan's upload, tile descriptors, the launches, verdicts and side data.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "devbatch.hpp"

#define HIPCHK(x)                             \
  do {                                        \
    hipError_t _e = (x);                      \
    if (_e != hipSuccess) return KW_E_DEVICE; \
  } while (0)

namespace kw {

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

// Diagnostics (KW_BULK_DEBUG): the device time between two points of a stream, by timing events of
// its own; off, every call is a no-op (summary.cpp, outcomes.cpp print it: scripts/metrics_pass_bench.py).
struct StreamTimer {
  hipEvent_t a = nullptr, b = nullptr;
  bool on;
  explicit StreamTimer(bool want) : on(want) {
    if (on) on = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess;
  }
  StreamTimer(const StreamTimer&) = delete;
  ~StreamTimer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  void start(hipStream_t s) {
    if (on) (void)hipEventRecord(a, s);
  }
  void stop(hipStream_t s) {
    if (on) (void)hipEventRecord(b, s);
  }
  double ms() {  // (waits for the second point)
    float t = 0;
    if (on && hipEventSynchronize(b) == hipSuccess) (void)hipEventElapsedTime(&t, a, b);
    return t;
  }
};

// The environment's compiled tables to `device` (< 0: host only).
int upload_env(kw_env* env, int device);

// The descriptors of tiles [t0, t1) of geometry T over rows [lo, hi), in row order, and the requests that exceed the
// capacities alone (overflow); a run that does not fit is halved until its parts do. Tiles in ranges
// of `range` on the host workers. KW_E_ARG when an overflow request index exceeds u32.
// [t0, t1) counts tiles of the full height T.rows, which fixes the rows covered; with KW_TILE_CUT
// (the default) a range's rows are cut into tiles of [rows - rows / 8, rows] rows each, at the least
// estimated cost per row, so a range gives up to 1/8 more descriptors than tiles. A range keeps the
// fixed cut where that is the cheaper, and the whole call does where the cuts would give the busiest
// slot of a launch of `grid` workgroups over these descriptors a tile more. grid 0 (the bulk path's
// per-chunk descriptors) and launches of the image families alone: the fixed cut.
int build_descs(const Batch& B, const TileArgs& T, uint64_t lo, uint64_t hi, uint64_t t0, uint64_t t1, uint64_t range,
                uint32_t grid, std::vector<TileDesc>* desc, std::vector<uint32_t>* ovf);

// A descriptor's estimated cost (kernels.hpp tile_cost over its item counts); one the host queued
// for the overflow kernels (fits == 0) costs the tile kernel nothing.
uint64_t desc_cost(const TileCostW& w, const TileDesc& d);

// A resident pass's descriptors, region after region (at[k], nd[k]: region k's place and count),
// cut by build_descs, in row order; one overflow list ([count, rows...]).
int plan_descs(const Batch& B, const PassPlan& plan, std::vector<TileDesc>* desc, std::vector<uint32_t>* ovf, uint64_t at[2],
               uint64_t nd[2]);

// Per-string class arrays of the overflow path (absolute entity indices), one allocation.
int ensure_overflow_classes(const Batch& B, DeviceBatch* D, const TileArgs& T, EvalArgs* A);

// Everything a pass's launches need on the device before the first one: the plan's records and
// TileArgs, the rows-mode column map, tile descriptors and overflow list, schedule counters and the
// side-data buffers; *out_args: the launch arguments. descs false: the caller builds and uploads
// descriptors per row chunk (bulk.cpp).
int prepare_pass(kw_batch* kb, PassPlan& plan, hipStream_t s, EvalArgs* out_args, bool descs = true);

// A planned pass with its wide policy groups (PassPlan::wide): their members first run as a
// separate all-pairs pass into member_words, then the pass itself (wide columns hold a
// placeholder), then the combine kernel writes those columns and their cause bitsets. The member
// pass's own side data (entity indices >= 65535 of members) is not kept: the main pass reuses the
// buffers. `timed`: HIP events bracket the main pass.
int run_validate(const kw_env* env, kw_batch* kb, PassPlan& plan, int origin, bool timed, hipStream_t s);

// The checks of a pass's arguments, its verdict buffer and its plan (all pairs, or rows mode when
// row_policy is given).
int validate_common(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, const int32_t* row_policy,
                    int origin, PassPlan* plan);

// validate_common for an all-pairs pass through the batch's plan cache (DeviceBatch::plan_cache):
// a repeated pass (same environment, policy list, origin and KW_* settings) skips planning; the
// checks and the verdict buffer are redone every time.
int validate_cached(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, PassPlan** out);

// kw_validate_timed: `reps` passes bracketed by HIP events after `warmup` untimed ones.
int validate_timed(const kw_env* env, kw_batch* b, const int32_t* policies, uint32_t npol, int origin, int warmup, int reps,
                   kw_timing* out);

// The pass's side data into the batch's host copy (kw_batch_wide_arg, the formatter): entity
// indices >= 65535 and > 15-member group causes (kernels.hpp WideRec), after the pass on stream s.
int load_side_data(kw_batch* b, hipStream_t s);

// kw_batch_verdicts: the first `count` verdict words of the last pass in batch-row order, then the
// side data.
int read_verdicts(kw_batch* b, uint32_t* host_out, size_t count);

// The messages of chosen findings (messages.cpp): kw_batch_messages over the last all-pairs pass,
// and the host renderers and the statistics of the diagnostics.
int batch_messages(kw_batch* b, const kw_env* env, const int32_t* policies, uint32_t npol, const uint64_t* rows,
                   const uint32_t* cols, size_t n, kw_messages* out);
int debug_messages_words(const kw_env* env, const kw_batch* b, const int32_t* policies, uint32_t npol, const uint32_t* words,
                         uint64_t nrows, const uint64_t* rows, const uint32_t* cols, size_t n, int how, kw_messages* out);
int debug_messages_stats(const kw_batch* b, uint64_t* out);
// The container names to the device on stream s (DeviceBatch::names; the messages and the responses
// upload them on first use).
int upload_names(kw_batch* kb, hipStream_t s);

// The AdmissionResponse bodies of chosen pairs (responses.cpp): kw_batch_responses over the last
// all-pairs pass, and the host renderers and the statistics of the diagnostics.
int batch_responses(kw_batch* b, const kw_env* env, const int32_t* policies, uint32_t npol, const uint64_t* rows,
                    const uint32_t* cols, size_t n, kw_responses* out);
int debug_responses_words(const kw_env* env, const kw_batch* b, const int32_t* policies, uint32_t npol, const uint32_t* words,
                          uint64_t nrows, const uint64_t* rows, const uint32_t* cols, size_t n, int how, kw_responses* out);
int debug_responses_stats(const kw_batch* b, uint64_t* out);

// The JSONPatch of accepted mutations from columns (patches.cpp): the patch-shape columns,
// kw_batch_patches over the last all-pairs pass, and the host renderers and the statistics of the
// diagnostics.
int batch_set_patch_shape(kw_batch* b, const uint32_t* ctr_place, uint64_t n_containers, const uint8_t* req_place, uint64_t n_requests);
int batch_patch_shape(const kw_batch* b, uint32_t* ctr_place, uint64_t n_containers, uint8_t* req_place, uint64_t n_requests);
int batch_patches(kw_batch* b, const kw_env* env, const int32_t* policies, uint32_t npol, const uint64_t* rows, const uint32_t* cols,
                  size_t n, int form, kw_responses* out);
int debug_patches_words(const kw_env* env, const kw_batch* b, const int32_t* policies, uint32_t npol, const uint32_t* words,
                        uint64_t nrows, const uint64_t* rows, const uint32_t* cols, size_t n, int form, int how, kw_responses* out);
int debug_patches_stats(const kw_batch* b, uint64_t* out);

}  // namespace kw
