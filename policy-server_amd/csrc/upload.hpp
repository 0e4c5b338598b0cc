// upload.hpp — the host batch to the device image (upload.cpp): the light / heavy row split, the
// image's layout in pieces, the whole-batch upload, and the bulk host -> host pass that uploads,
// evaluates and reads back in row chunks (bulk.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "devbatch.hpp"

namespace kw {

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

// The columns of the device image, in image order: fn(kind, m, ptr, bytes) for the six row /
// container arrays (m = -1), then `off` and `bytes` of each string column m. The one list that the
// layout, the page-locking and the planner's host view all follow.
template <typename F>
void for_each_column(const Batch& B, F&& fn) {
  fn(PK_ROW_U8, -1, (const void*)B.req_flags.data(), B.req_flags.size());
  fn(PK_ROW_OFF, -1, (const void*)B.ctr_off.data(), B.ctr_off.size() * 4);
  fn(PK_ROW_OFF, -1, (const void*)B.lbl_off.data(), B.lbl_off.size() * 4);
  fn(PK_CTR_U8, -1, (const void*)B.ctr_flags.data(), B.ctr_flags.size());
  fn(PK_CTR_OFF, -1, (const void*)B.capadd_off.data(), B.capadd_off.size() * 4);
  fn(PK_CTR_OFF, -1, (const void*)B.capdrop_off.data(), B.capdrop_off.size() * 4);
  for (int m = 0; m < (int)NSTR; ++m) {
    const StrCol& c = host_str(B, m);
    fn(PK_STR_OFF, m, (const void*)c.off.data(), c.off.size() * 4);
    fn(PK_STR_BYTES, m, (const void*)c.bytes.data(), c.bytes.size());
  }
}

// The light region's row count and the device-row order (perm[d] = batch row), or 0 when the batch
// stays in order: the heavy rows must be between 1 % and 50 % of the rows and hold at least 30 % of
// the containers, in a batch of at least 2^18 rows. KW_SPLIT=0 never splits, KW_SPLIT=1
// splits whenever both regions are non-empty (tests).
uint64_t split_rows(const Batch& B, std::vector<uint64_t>* perm);

// Batch rows in `perm` order as a new batch (P's row d = B's row perm[d]). with_bytes false: the
// device string columns get their offsets only — the upload gathers their bytes straight into its
// staging (gather_column) — and the host-only string columns stay empty. *order: the entity maps.
void permute_batch(const Batch& B, const std::vector<uint64_t>& perm, Batch* P, bool with_bytes, RowOrder* order);

// Allocates the batch's device image (one pooled allocation, 256-B aligned sub-arrays) and its
// pinned staging block, and points the DeviceBatch views at it; nothing is copied.
int layout_batch(kw_batch* kb, int device, hipStream_t stream, std::vector<Piece>* pieces, bool may_split = false,
                 bool staging = true);

// Upload the batch's columns to `device`: one pooled allocation with 256-B aligned sub-arrays,
// assembled in pinned host staging and copied with one async H2D on `stream` (null: a new stream
// owned by the batch); `sync` waits for the copy.
int upload_batch(kw_batch* kb, int device, hipStream_t stream, bool sync);

// Byte range [lo, hi) of piece p that rows [r0, r1) occupy. A chunk's string bytes run 64 bytes past
// its last string (the device's batched reads past a string end stay inside uploaded bytes); the
// first chunk starts at 0 and the last runs to the piece's end (its zero padding).
void piece_range(const Batch& B, const Piece& p, uint64_t r0, uint64_t r1, bool last, size_t* lo, size_t* hi);

// kw_batch_pin_host: page-locks the batch's column arrays in place (those of 64 KiB and more).
int pin_host(kw_batch* kb, int device);

// A host view of the batch for planning alone (kw_debug_plan): no device memory, nothing launched,
// the columns in the device-row order kw_batch_to_device would give them. The caller clears
// `verdicts` (a host word, not the DeviceBatch's to free) before the view dies.
std::unique_ptr<DeviceBatch> host_view(kw_batch* kb);

// kw_validate_host (bulk.cpp).
int validate_host(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, int device,
                  uint32_t* out, size_t count, uint32_t chunk_rows);
// kw_validate_host_packed (bulk.cpp): the same pass, the verdicts in the packed form (packed.hpp).
int validate_host_packed(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, int device,
                         kw_packed* out, uint32_t chunk_rows);
// kw_validate_host_summary (bulk.cpp): the same pass, the summary form (summary.hpp) its only output.
int validate_host_summary(const kw_env* env, kw_batch* kb, const int32_t* policies, uint32_t npol, int origin, int device,
                          kw_summary* out, uint32_t chunk_rows);
// Whether p is page-locked host memory the copy engines reach directly.
bool page_locked(const void* p);
// The dictionary of a packed pass, dict [npol][3] (packed.cpp): a function of the environment, the
// policy list and the origin alone. KW_E_ARG for a policy index outside the visible policies.
int packed_dict(const Env& E, const int32_t* policies, uint32_t npol, int origin, uint32_t* dict);

}  // namespace kw
