// lastpass.cpp — the report drivers' call frame (lastpass.hpp) and the C entry point that sizes a
// caller's buffers by the last pass (include/kwgpu.h kw_batch_last_pass).
#include "lastpass.hpp"

namespace kw {

bool last_pass(const kw_batch* b, uint64_t* rows, uint32_t* rw) {
  if (!b || !b->dev || b->dev->device < 0) return false;
  const DeviceBatch& D = *b->dev;
  if (!D.last_row_words || !D.verdicts) return false;
  *rw = D.last_row_words;
  *rows = D.last_verdicts / D.last_row_words;
  return true;
}

LastPass::LastPass(kw_batch* b, Need need) {
  if (!last_pass(b, &rows, &npol)) return;
  DeviceBatch& D = *b->dev;
  if (need == kWholeBatch && (D.last_rows_mode || (rows >> 32) || rows != b->b.n || (D.split && D.perm.size() != rows))) return;
  dev = &D;
}

int LastPass::open() {
  HIPCHK(hipSetDevice(dev->device));
  drain_.s = s = dev->cur ? dev->cur : dev->stream;
  drain_.on = true;
  return KW_OK;
}

int upload_row_maps(LastPass& F, const uint32_t** d2b, const uint32_t** b2d) {
  DeviceBatch& D = *F.dev;
  *d2b = nullptr;
  if (b2d) *b2d = nullptr;
  if (!D.split) return KW_OK;
  const uint64_t rows = F.rows;
  const size_t bytes = (size_t)rows * (b2d ? 8 : 4);
  BlockLease &h = F.lease(), &d = F.lease();
  HIPCHK(h.alloc(host_pool(), D.device, bytes));
  HIPCHK(d.alloc(dev_pool(), D.device, bytes));
  uint32_t* m = (uint32_t*)h.p;
  for (uint64_t i = 0; i < rows; ++i) m[i] = (uint32_t)D.perm[i];
  if (b2d)
    for (uint64_t i = 0; i < rows; ++i) m[rows + i] = (uint32_t)D.device_rows()[i];
  HIPCHK(hipMemcpyAsync(d.p, h.p, bytes, hipMemcpyHostToDevice, F.s));
  *d2b = (const uint32_t*)d.p;
  if (b2d) *b2d = *d2b + rows;
  return KW_OK;
}

uint32_t resident_mask(const DigestCols& C) {
  uint32_t have = 0;
  for (uint32_t m = 0; m < DG_NSTR; ++m) have |= C.str[m].off ? 1u << m : 0u;
  return have;
}

int bounce_read(BlockLease& bounce, int device, hipStream_t s, void* dst, const void* src, size_t bytes) {
  if (!bounce.p) HIPCHK(bounce.alloc(host_pool(), device, std::min(kBounce, std::max<size_t>(bytes, 4096))));
  for (size_t at = 0, k; at < bytes; at += k) {
    k = std::min(bounce.bytes, bytes - at);
    HIPCHK(hipMemcpyAsync(bounce.p, (const uint8_t*)src + at, k, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    parallel_copy((uint8_t*)dst + at, bounce.p, k);
  }
  return KW_OK;
}

}  // namespace kw

extern "C" int kw_batch_last_pass(const kw_batch* b, uint64_t* rows, uint32_t* row_words) {
  if (!rows || !row_words) return KW_E_ARG;
  return kw::last_pass(b, rows, row_words) ? KW_OK : KW_E_ARG;
}
