// bulkplan.hpp — the pure arithmetic of the bulk path (bulk.cpp): the chunk schedule, the slab
// schedule of an unchunked pass, the depth of chunks in flight and the packed layout of a chunk's
// staged ranges. No HIP, no batch, no settings: values of KW_* settings come in as arguments
// (tests/bulkplan_check.cpp runs it on the host).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace kw {

// Tiles of a full chunk: `per_rows` rows, at least one tile, and enough that the batch takes at
// most ~240 chunks (the events and the host's per-chunk work stay bounded).
inline uint64_t chunk_tiles(uint64_t ntiles, uint64_t tile_rows, uint64_t per_rows) {
  return std::max<uint64_t>({1, per_rows / tile_rows, (ntiles + 239) / 240});
}

// Chunk k of a bulk pass covers tiles [tb[k], tb[k+1]). The read-back stream is the longest (4 B x
// npol per request out vs the request's columns in), so with `ramp` the first chunks are small
// (1/16 of a full chunk, doubling) to start it early. The last chunks shrink the same way (r05):
// the final chunk's read-back overlaps nothing, so a full-size last chunk left ~1 ms of C4's
// read-back exposed.
inline std::vector<uint64_t> chunk_bounds(uint64_t ntiles, uint64_t tile_rows, uint64_t per_rows, bool ramp) {
  const uint64_t tper = chunk_tiles(ntiles, tile_rows, per_rows);
  std::vector<uint64_t> tb{0};
  std::vector<uint64_t> head, tail;  // chunk sizes in tiles, from the front and from the back
  uint64_t left = ntiles, sh = ramp ? std::max<uint64_t>(1, tper / 16) : tper, st = sh;
  while (left) {
    head.push_back(std::min(sh, left));
    left -= head.back();
    sh = std::min(tper, sh * 2);
    if (!left || !ramp) continue;
    tail.push_back(std::min(st, left));
    left -= tail.back();
    st = std::min(tper, st * 2);
  }
  for (uint64_t h : head) tb.push_back(tb.back() + h);
  for (auto it = tail.rbegin(); it != tail.rend(); ++it) tb.push_back(tb.back() + *it);
  return tb;
}

// The row slabs in which the packed and the summary form go through the verdict buffer of a pass
// that ran unchunked: slab k covers rows [rb[k], rb[k+1]), `per_rows` rows each, at least one, and
// enough that there are at most 240; no rows: the single bound {0}, no slab.
inline std::vector<uint64_t> slab_bounds(uint64_t rows, uint64_t per_rows) {
  const uint64_t slab = std::max<uint64_t>({1, per_rows, (rows + 239) / 240});
  std::vector<uint64_t> rb;
  for (uint64_t r = 0; r < rows; r += slab) rb.push_back(r);
  rb.push_back(rows);
  return rb;
}

// Pinned output: at most this many chunks in flight past the read-back (0: unbounded). Unbounded,
// the host queues every chunk's copies and launch at once and the copies run slower (C4 1M:
// 16.0-16.7 ms vs 9.7-10.9 at depth 2, profiles/r04_bulk_modes.txt). Staged columns take 3 (the
// host fills pace the uploads), columns DMA'd in place 2 (at 3 their uploads crowd the read-backs:
// 11.0 vs 7.1 ms, profiles/r04_bulk_sweep.txt). depth_knob (KW_BULK_DEPTH) >= 0 overrides.
inline uint64_t bulk_depth(int depth_knob, bool any_dma) {
  return depth_knob >= 0 ? (uint64_t)depth_knob : (any_dma ? 2 : 3);
}

// A byte range of the device image: where it starts there and its length.
struct PackRange {
  uint64_t dev_off, len;
};

// The chunk's staged ranges (piece order) packed into one slot: range i at (*at)[i], each at its
// device offset's residue mod 16 after the previous range's end rounded up to 16 (the scatter
// kernel moves aligned 16-byte words). Returns the packed bytes.
inline uint64_t pack_ranges(const std::vector<PackRange>& r, std::vector<uint64_t>* at) {
  uint64_t pk = 0;
  at->clear();
  for (const PackRange& x : r) {
    at->push_back(((pk + 15) & ~(uint64_t)15) + (x.dev_off & 15));
    pk = at->back() + x.len;
  }
  return pk;
}

// Slot bytes that hold pack_ranges' result for these ranges: per range at most 15 B up to the next
// 16 and 15 B of residue, so len + 32 each; 256-B granules.
inline uint64_t slot_estimate(const std::vector<PackRange>& r) {
  uint64_t b = 0;
  for (const PackRange& x : r) b += x.len + 32;
  return (b + 255) & ~(uint64_t)255;
}

}  // namespace kw
