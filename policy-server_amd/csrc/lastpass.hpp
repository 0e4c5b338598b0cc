// lastpass.hpp — the call frame the reports over a resident pass share (summary.cpp, outcomes.cpp,
// digest.cpp, members.cpp, messages.cpp; lastpass.cpp): the last pass and the checks on it, its
// device and stream, the call's pooled blocks and the drain before their release, a split batch's
// row maps, the bounce read-back.
#pragma once
#include <chrono>
#include <deque>

#include "devbatch.hpp"
#include "pass.hpp"

namespace kw {

// The rows of the last pass and its words per row; false when the batch holds no pass.
bool last_pass(const kw_batch* b, uint64_t* rows, uint32_t* row_words);

inline double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}
constexpr size_t round_up(size_t n, size_t a) { return (n + a - 1) & ~(a - 1); }  // a: a power of two

// Destroyed before the blocks a call holds: the stream is drained before any block returns to its
// pool, on the error returns too.
struct Drain {
  hipStream_t s = nullptr;
  bool on = false;
  ~Drain() { if (on) (void)hipStreamSynchronize(s); }
};

// What a driver constructs first. The constructor resolves the last pass and touches no device:
// ok() is false where the driver answers KW_E_ARG. kWholeBatch asks for an all-pairs pass over every
// row of the batch, rows as u32 (digest, members, messages). open() selects the pass's device and
// stream; from then on the frame's end drains the stream before the blocks taken through lease() go
// back to their pools, whichever return the driver leaves by.
struct LastPass {
  enum Need { kAnyPass, kWholeBatch };
  uint64_t rows = 0;
  uint32_t npol = 0;  // verdict words per row
  DeviceBatch* dev = nullptr;
  hipStream_t s = nullptr;
  LastPass(kw_batch* b, Need need);
  bool ok() const { return dev != nullptr; }
  int open();
  BlockLease& lease() { return blocks_.emplace_back(); }

 private:
  std::deque<BlockLease> blocks_;
  Drain drain_;  // (after blocks_: destroyed first)
};

// A split batch's row maps as u32 on the device, through blocks of the frame on its stream: *d2b the
// batch row of each device row, *b2d (when asked for) the reverse. Not split: nullptr, no upload.
int upload_row_maps(LastPass& F, const uint32_t** d2b, const uint32_t** b2d = nullptr);

// The string columns (bits of Str) that `C` holds.
uint32_t resident_mask(const DigestCols& C);

// Device bytes to a pageable host buffer through a pinned block of at most kBounce bytes (allocated
// on first use, good for several calls) and parallel_copy; every copy is synchronised on return.
constexpr size_t kBounce = (size_t)64 << 20;
int bounce_read(BlockLease& bounce, int device, hipStream_t s, void* dst, const void* src, size_t bytes);

}  // namespace kw
