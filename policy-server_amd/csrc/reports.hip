// reports.hip — the kernels of the reports over a resident pass's verdict words (reports.hpp). A
// translation unit of its own: none of them uses the hot path's device code (kernels.hip), so a
// change here does not recompile the tile kernel's instantiations, nor the reverse.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/kwgpu.h"
#include "reports.hpp"

namespace kw {

// ---- building blocks -------------------------------------------------------------------------------
// (64-bit values go through the runtime's own 64-bit __shfl / __shfl_up / __shfl_down overloads.)

// Exclusive scan of v over the workgroup's THREADS threads (*total: their sum): a wave scan by
// shuffles, the waves' totals through lds (THREADS / 64 values). Every thread calls it. One barrier
// between the waves' writes and the reads, one after the reads: lds is free on return, for the next
// call or anything else. (The pack kernels' scan had its second barrier ahead of the writes, against
// the reads of a call before; their calls in a loop touch lds nowhere else, so the barrier that ends
// call k orders the same reads before the same writes of call k + 1.)
template <typename T, uint32_t THREADS>
__device__ inline T block_scan(T v, T* lds, T* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  T upto = v;
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const T o = __shfl_up(upto, d);
    if (lane >= d) upto += o;
  }
  if (lane == 63u) lds[wave] = upto;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < THREADS / 64u; ++w) {
    const T s = lds[w];
    before += w < wave ? s : (T)0;
    all += s;
  }
  __syncthreads();
  *total = all;
  return before + (upto - v);
}

// The middle launch of a scan in three: one workgroup turns n totals into their bases in place
// (sums[i] = carry + the totals before i), THREADS x PER of them a round, and returns the end.
template <typename T, uint32_t THREADS, uint32_t PER>
__device__ inline T scan_bases(T* sums, uint32_t n, T carry, T* lds) {
  for (uint32_t r0 = 0; r0 < n; r0 += THREADS * PER) {  // uniform (every thread keeps the same carry)
    const uint32_t i = r0 + PER * threadIdx.x;
    T l[PER], mine = 0, total;
#pragma unroll
    for (uint32_t j = 0; j < PER; ++j) {
      l[j] = i + j < n ? sums[i + j] : (T)0;
      mine += l[j];
    }
    T at = carry + block_scan<T, THREADS>(mine, lds, &total);
#pragma unroll
    for (uint32_t j = 0; j < PER; ++j) {
      if (i + j < n) sums[i + j] = at;
      at += l[j];
    }
    carry += total;
  }
  return carry;
}

// ---- packed verdict output (reports.hpp PackArgs, packed.hpp) -----------------------------------

// What a lane holds in round t of a pack kernel's wave: its item, and its column when it holds one.
struct PackLane {
  uint64_t item, row;
  uint32_t col, c, sub;
  bool on;
};
__device__ inline PackLane pack_lane(const PackArgs& a, const PackGeom& g, uint64_t item0, uint32_t t, uint32_t lane) {
  PackLane L;
  L.sub = lane / g.w;
  L.c = lane % g.w;
  L.item = item0 + (uint64_t)t * g.ipi + L.sub;
  const uint32_t grp = a.G == 1u ? 0u : (uint32_t)(L.item % a.G);
  L.row = a.G == 1u ? L.item : L.item / a.G;
  L.col = 64u * grp + L.c;
  L.on = L.sub < g.ipi && L.item < a.nitems && L.col < a.npol;
  return L;
}

__global__ void __launch_bounds__(256) pack_codes_kernel(PackArgs a) {
  const PackGeom g = pack_geom(a.npol);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t item0 = ((((uint64_t)blockIdx.x * 256u) + threadIdx.x) >> 6) * g.ipw;  // wave-uniform
  if (item0 >= a.nitems) return;
  const uint64_t mask = g.w == 64u ? ~0ull : (1ull << g.w) - 1ull;
  uint32_t d0 = 0, d1 = 0, d2 = 0, dcol = ~0u;  // the lane's column's dictionary
  uint64_t my_lo = 0, my_hi = 0;
  for (uint32_t t = 0; t < g.T; ++t) {
    const PackLane L = pack_lane(a, g, item0, t, lane);
    uint32_t code = 0;
    if (L.on) {
      if (L.col != dcol) {  // (only passes of more than 64 columns change a lane's column)
        dcol = L.col;
        d0 = a.dict[3u * dcol], d1 = a.dict[3u * dcol + 1u], d2 = a.dict[3u * dcol + 2u];
      }
      code = packed_code(a.words[L.row * a.npol + L.col], d0, d1, d2);
    }
    const uint64_t blo = __ballot(code & 1u), bhi = __ballot(code >> 1);
    const uint32_t j = lane - t * g.ipi;  // lane t * ipi + j keeps the round's item j
    if (lane >= t * g.ipi && j < g.ipi) {
      my_lo = (blo >> (j * g.w)) & mask;
      my_hi = (bhi >> (j * g.w)) & mask;
    }
  }
  if (lane < g.ipw && item0 + lane < a.nitems) {
    *(ulonglong2*)(a.planes + 2u * (item0 + lane)) = make_ulonglong2(my_lo, my_hi);
    a.ibase[item0 + lane] = packed_popc(my_lo & my_hi);
  }
}

__global__ void __launch_bounds__(256) pack_sums_kernel(PackArgs a) {
  __shared__ uint32_t lds[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x * kScanPer;
  uint32_t s = 0;
  for (uint32_t q = 0; q < kScanPer; ++q)
    if (i0 + q < a.nitems) s += a.ibase[i0 + q];
  uint32_t total;
  (void)block_scan<uint32_t, 256>(s, lds, &total);
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) pack_scan_kernel(PackArgs a, uint32_t nblocks) {  // one workgroup
  __shared__ uint32_t lds[4];
  const uint32_t carry = scan_bases<uint32_t, 256, 1>(a.bsum, nblocks, a.tot[0], lds);
  if (threadIdx.x == 0) {
    a.tot[1] = carry;
    a.exc_off[a.nitems / a.G] = carry;
  }
}

__global__ void __launch_bounds__(256) pack_bases_kernel(PackArgs a) {
  __shared__ uint32_t lds[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x * kScanPer;
  uint32_t c[kScanPer], s = 0;
  for (uint32_t q = 0; q < kScanPer; ++q) {
    c[q] = i0 + q < a.nitems ? a.ibase[i0 + q] : 0u;
    s += c[q];
  }
  uint32_t total;
  uint32_t at = a.bsum[blockIdx.x] + block_scan<uint32_t, 256>(s, lds, &total);
  for (uint32_t q = 0; q < kScanPer; ++q) {
    const uint64_t i = i0 + q;
    if (i < a.nitems) {
      a.ibase[i] = at;
      if (a.G == 1u) a.exc_off[i] = at;
      else if (i % a.G == 0) a.exc_off[i / a.G] = at;
    }
    at += c[q];
  }
}

__global__ void __launch_bounds__(256) pack_scatter_kernel(PackArgs a) {
  const PackGeom g = pack_geom(a.npol);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t item0 = ((((uint64_t)blockIdx.x * 256u) + threadIdx.x) >> 6) * g.ipw;
  if (item0 >= a.nitems) return;
  const uint32_t seed = a.tot[0];
  for (uint32_t t = 0; t < g.T; ++t) {
    const PackLane L = pack_lane(a, g, item0, t, lane);
    if (!L.on) continue;
    const ulonglong2 pl = *(const ulonglong2*)(a.planes + 2u * L.item);
    const uint64_t esc = pl.x & pl.y;
    if (!((esc >> L.c) & 1ull)) continue;
    const uint32_t at = a.ibase[L.item] - seed + packed_popc(esc & packed_below(L.c));
    if (at < a.exc_cap) a.exc[at] = a.words[L.row * a.npol + L.col];
  }
}

hipError_t launch_pack(const PackArgs& a, hipStream_t s) {
  if (a.nitems == 0) return hipSuccess;
  const PackGeom g = pack_geom(a.npol);
  const uint64_t waves = ((uint64_t)a.nitems + g.ipw - 1u) / g.ipw;
  const uint32_t wgrid = (uint32_t)((waves + 3u) / 4u);
  const uint32_t nb = (uint32_t)(((uint64_t)a.nitems + kScanBlock - 1u) / kScanBlock);
  hipLaunchKernelGGL(pack_codes_kernel, dim3(wgrid), dim3(256), 0, s, a);
  hipLaunchKernelGGL(pack_sums_kernel, dim3(nb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(256), 0, s, a, nb);
  hipLaunchKernelGGL(pack_bases_kernel, dim3(nb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(pack_scatter_kernel, dim3(wgrid), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- summary form (reports.hpp SumArgs, summary.hpp) --------------------------------------------

#ifndef KW_SUM_LDS  // the 17 reason buckets: 1 a per-wave LDS table, 0 compare-and-add in registers (build-time A/B)
#define KW_SUM_LDS 1
#endif
constexpr uint32_t kSumBuckets = 17;  // reasons 0..15 and "other"; odd, so also the LDS table's row stride

__global__ void __launch_bounds__(256) summary_kernel(SumArgs a, SumGeom g) {
  __shared__ uint32_t wg[64 * KW_SUM_N];  // the workgroup's partial block
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, grp = blockIdx.y;
  for (uint32_t i = threadIdx.x; i < 64u * KW_SUM_N; i += 256u) wg[i] = 0;
#if KW_SUM_LDS
  __shared__ uint32_t rs[kSumWaves * 64 * kSumBuckets];
  uint32_t* mine = rs + (wave * 64u + lane) * kSumBuckets;
  for (uint32_t b = 0; b < kSumBuckets; ++b) mine[b] = 0;
#else
  uint32_t mine[kSumBuckets];
#pragma unroll
  for (uint32_t b = 0; b < kSumBuckets; ++b) mine[b] = 0;
#endif
  __syncthreads();
  const uint32_t w = g.p.w, ipi = g.p.ipi, T = g.p.T;
  const uint32_t sub = lane / w, c = lane % w, col = 64u * grp + c;
  const bool lane_on = sub < ipi && col < a.npol;  // (sum_lane's column part: fixed for the kernel)
  const uint64_t mask = w == 64u ? ~0ull : (1ull << w) - 1ull;
  const uint64_t nwaves = (uint64_t)kSumWaves * gridDim.x;
  const bool planes = a.planes != nullptr;
  uint32_t n_fa = 0, n_va = 0, n_vm = 0, n_fp = 0, n_by = 0, n_s1 = 0, n_s2 = 0, n_s3 = 0;
  for (uint64_t unit = (uint64_t)blockIdx.x * kSumWaves + wave; unit < g.units; unit += nwaves) {  // wave-uniform
    const uint64_t row0 = unit * g.p.ipw;
    // the unit's words first: up to kSumRounds loads in flight per lane
    uint32_t x[kSumRounds], onm = 0;
#pragma unroll
    for (uint32_t t = 0; t < kSumRounds; ++t) {
      const SumLane L = sum_lane(g, a.rows, a.npol, grp, unit, t, lane);
      x[t] = L.on ? __builtin_nontemporal_load(a.words + L.row * a.npol + L.col) : 0u;
      onm |= (L.on ? 1u : 0u) << t;
    }
    uint64_t my_lo = 0, my_hi = 0;
#pragma unroll
    for (uint32_t t = 0; t < kSumRounds; ++t) {
      if (t >= T) continue;  // wave-uniform (not a break: the loop unrolls fully, x[t] stays a register)
      const uint32_t v = x[t];
      const bool on = (onm >> t) & 1u;
      // (a lane that holds no word has v = 0: no flag, status None)
      n_fa += (v >> 2) & 1u;
      n_va += v & 1u;
      n_vm += (v >> 1) & 1u;
      n_fp += (v >> 6) & 1u;
      n_by += (v >> 5) & 1u;
      const uint32_t st = (v & KW_F_STATUS_MASK) >> KW_F_STATUS_SHIFT;
      n_s1 += st == 1u ? 1u : 0u;
      n_s2 += st == 2u ? 1u : 0u;
      n_s3 += st == 3u ? 1u : 0u;
      const uint32_t r = KW_REASON(v), b = r < kSumBuckets - 1u ? r : kSumBuckets - 1u;
#if KW_SUM_LDS
      if (on) __hip_atomic_fetch_add(mine + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
#else
#pragma unroll
      for (uint32_t q = 0; q < kSumBuckets; ++q) mine[q] += on && b == q ? 1u : 0u;
#endif
      if (planes) {
        const uint64_t blo = __ballot(on && sum_bit_reject(v)), bhi = __ballot(on && sum_bit_found(v));
        const uint32_t j = lane - t * ipi;  // lane t * ipi + j keeps the round's row j
        if (lane >= t * ipi && j < ipi) {
          my_lo = (blo >> (j * w)) & mask;
          my_hi = (bhi >> (j * w)) & mask;
        }
      }
    }
    if (planes && lane < g.p.ipw && row0 + lane < a.rows)
      *(ulonglong2*)(a.planes + 2u * ((row0 + lane) * g.G + grp)) = make_ulonglong2(my_lo, my_hi);
  }
  // the waves of the workgroup, and the lanes that share a column, into the partial block
  if (lane_on) {
    uint32_t* d = wg + c * KW_SUM_N;
    auto add = [d](uint32_t k, uint32_t n) {
      if (n) __hip_atomic_fetch_add(d + k, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    add(KW_SUM_F_ALLOWED, n_fa), add(KW_SUM_V_ALLOWED, n_va), add(KW_SUM_V_MUTATED, n_vm), add(KW_SUM_F_PATCH, n_fp);
    add(KW_SUM_BYPASS, n_by), add(KW_SUM_FST_VANILLA, n_s1), add(KW_SUM_FST_MUTATION_REFUSED, n_s2);
    add(KW_SUM_FST_INIT_ERROR, n_s3);
#pragma unroll
    for (uint32_t b = 0; b + 1u < kSumBuckets; ++b) add(KW_SUM_REASON + b, mine[b]);
    add(KW_SUM_REASON_OTHER, mine[kSumBuckets - 1u]);
  }
  __syncthreads();
  uint32_t* out = a.part + ((uint64_t)grp * gridDim.x + blockIdx.x) * g.cols * KW_SUM_N;
  for (uint32_t i = threadIdx.x; i < g.cols * KW_SUM_N; i += 256u) out[i] = wg[i];
}

// A workgroup per column: its 256 threads are kSumSlices slices of the column's KW_SUM_N counters,
// slice q sums the partial blocks q, q + kSumSlices, ... (four loads in flight a thread), and one
// thread per counter adds the slices in order into the running total. (One thread per counter over
// all the blocks — 2048 threads on the whole device for 64 columns — took 105 us a launch, four times
// the reduction itself: profiles/r10_summary.txt.)
constexpr uint32_t kSumSlices = 256 / KW_SUM_N;
__global__ void __launch_bounds__(256) summary_totals_kernel(SumArgs a, SumGeom g) {
  __shared__ uint64_t sl[kSumSlices][KW_SUM_N];
  const uint32_t col = blockIdx.x, k = threadIdx.x % KW_SUM_N, q = threadIdx.x / KW_SUM_N;
  const uint32_t grp = col / 64u, c = col - 64u * grp;
  const uint64_t stride = (uint64_t)g.cols * KW_SUM_N;
  const uint32_t* p = a.part + (uint64_t)grp * g.grid_x * stride + c * KW_SUM_N + k;
  uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  uint32_t x = q;
  for (; x + 3u * kSumSlices < g.grid_x; x += 4u * kSumSlices) {
    s0 += p[x * stride];
    s1 += p[(x + kSumSlices) * stride];
    s2 += p[(x + 2u * kSumSlices) * stride];
    s3 += p[(x + 3u * kSumSlices) * stride];
  }
  for (; x < g.grid_x; x += kSumSlices) s0 += p[x * stride];
  sl[q][k] = s0 + s1 + s2 + s3;
  __syncthreads();
  if (q == 0) {
    uint64_t s = 0;
    for (uint32_t j = 0; j < kSumSlices; ++j) s += sl[j][k];
    a.tot[col * (uint32_t)KW_SUM_N + k] += s;
  }
}

namespace {
uint32_t device_cus() {
  thread_local int c_dev = -1, c_ncu = 0;
  int dev = 0;
  if (hipGetDevice(&dev) == hipSuccess && dev != c_dev) {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) ncu = 0;
    c_dev = dev;
    c_ncu = ncu;
  }
  return (uint32_t)std::max(c_ncu, 0);
}
}  // namespace

size_t summary_part_bytes(uint64_t rows, uint32_t npol) {
  return (size_t)sum_part_words(sum_geom(rows, npol, device_cus())) * sizeof(uint32_t);
}

hipError_t launch_summary(const SumArgs& a, hipStream_t s) {
  if (a.rows == 0 || a.npol == 0) return hipSuccess;
  const SumGeom g = sum_geom(a.rows, a.npol, device_cus());
  if (sum_wg_rows(g) >> 32) return hipErrorInvalidValue;  // (sum_geom keeps it below: tests/summary_check.cpp)
  hipLaunchKernelGGL(summary_kernel, dim3(g.grid_x, g.G), dim3(256), 0, s, a, g);
  hipLaunchKernelGGL(summary_totals_kernel, dim3(a.npol), dim3(256), 0, s, a, g);
  return hipGetLastError();
}

__global__ void __launch_bounds__(256) gather_rows_kernel(GatherArgs a) {
  const uint64_t nw = a.n * a.row_words, nt = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nw; i += nt)
    a.out[i] = a.words[a.rows[i / a.row_words] * a.row_words + i % a.row_words];
}

hipError_t launch_gather_rows(const GatherArgs& a, hipStream_t s) {
  if (a.n == 0 || a.row_words == 0) return hipSuccess;
  const uint64_t nw = a.n * a.row_words;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((uint32_t)std::min<uint64_t>(4096, (nw + 255u) / 256u)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- grouped outcome count (reports.hpp OutcomeArgs, outcomes.hpp) -------------------------------

__global__ void __launch_bounds__(256) outcomes_kernel(OutcomeArgs a, PackGeom p) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, grp = blockIdx.y;
  const uint32_t unit = blockIdx.x * kOutWaves + wave;  // wave-uniform
  if (unit >= a.nunits) return;
  const OutUnit u = a.units[unit];
  const uint32_t rounds = out_rounds(p, u.n);
  uint32_t cnt[KW_OUT_N];
#pragma unroll
  for (uint32_t k = 0; k < (uint32_t)KW_OUT_N; ++k) cnt[k] = 0;
  for (uint32_t t0 = 0; t0 < rounds; t0 += kOutLoads) {  // wave-uniform
    // the rows of kOutLoads rounds first, then their words: that many loads in flight per lane
    uint32_t row[kOutLoads], x[kOutLoads], onm = 0;
#pragma unroll
    for (uint32_t i = 0; i < kOutLoads; ++i) {
      const OutLane L = out_lane(p, a.npol, grp, u.n, t0 + i, lane);
      row[i] = L.on ? a.order[u.first + L.entry] : 0u;
      onm |= (L.on ? 1u : 0u) << i;
    }
#pragma unroll
    for (uint32_t i = 0; i < kOutLoads; ++i)
      x[i] = (onm >> i) & 1u ? __builtin_nontemporal_load(a.words + (uint64_t)row[i] * a.npol + (64u * grp + lane % p.w)) : 0u;
#pragma unroll
    for (uint32_t i = 0; i < kOutLoads; ++i) {
      const uint32_t code = (onm >> i) & 1u ? outcome_code(x[i]) : (uint32_t)KW_OUT_N;
#pragma unroll
      for (uint32_t k = 0; k < (uint32_t)KW_OUT_N; ++k) cnt[k] += code == k ? 1u : 0u;
    }
  }
  // the unit into the table: a counter no lane holds is skipped by the whole wave; the lanes that
  // share a column (npol <= 32: lane c + s * w holds column c's rows of sub-row s) are summed into
  // lane c, whose adds of one outcome lie side by side in the table
  const uint32_t sub = lane / p.w, c = lane % p.w, col = 64u * grp + c;
  uint64_t* row_k = a.table + (uint64_t)(u.group - a.g0) * KW_OUT_N * a.npol + col;
#pragma unroll
  for (uint32_t k = 0; k < (uint32_t)KW_OUT_N; ++k) {
    if (!__ballot(cnt[k] != 0u)) continue;  // wave-uniform
    uint32_t tot = cnt[k];
    for (uint32_t s = 1; s < p.ipi; ++s) tot += (uint32_t)__shfl((int)cnt[k], (int)((c + s * p.w) & 63u));
    if (sub == 0u && col < a.npol && tot)
      __hip_atomic_fetch_add(row_k + (uint64_t)k * a.npol, (uint64_t)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

hipError_t launch_outcomes(const OutcomeArgs& a, hipStream_t s) {
  if (a.nunits == 0 || a.npol == 0) return hipSuccess;
  const uint32_t G = packed_groups(a.npol);
  if (G > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(outcomes_kernel, dim3((a.nunits + kOutWaves - 1u) / kOutWaves, G), dim3(256), 0, s, a, pack_geom(a.npol));
  return hipGetLastError();
}

// ---- violation digest (reports.hpp DigestArgs, digest.hpp) ---------------------------------------

constexpr uint64_t kDigestNone = ~0ull;

__device__ inline uint64_t digest_load(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void digest_overflow(const DigestArgs& a) {
  __hip_atomic_store(&a.head->overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The slot that holds `tag`, claimed when none does yet (claim); kDigestNone when the tag is absent or
// the probe gives up (which, claiming, marks the range as overflowed: the host cuts it).
__device__ inline uint64_t digest_slot(const DigestArgs& a, uint64_t tag, bool claim) {
  const uint64_t mask = a.nslots - 1u;
  uint64_t i = tag & mask;
  for (uint32_t probe = 0; probe < kDigestProbe; ++probe, i = (i + 1u) & mask) {
    // a range that has overflowed is cut and counted again: nothing more goes into its table, whose
    // probes would grow to kDigestProbe slots each past the load factor. Looked at on a long probe
    // only: one address read by every finding cost C4's count launch 19 ms (profiles/r14_digest.txt).
    if (claim && probe == 8u && __hip_atomic_load(&a.head->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return kDigestNone;
    uint64_t* tp = &a.table[i].tag;
    uint64_t t = digest_load(tp);
    if (t == 0u) {
      if (!claim) return kDigestNone;
      uint64_t expect = 0;
      if (__hip_atomic_compare_exchange_strong(tp, &expect, tag, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        const uint64_t n = __hip_atomic_fetch_add(&a.head->nclaimed, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n >= digest_max_groups(a.nslots)) digest_overflow(a);
        return i;
      }
      t = expect;
    }
    if (t == tag) return i;
  }
  if (claim) digest_overflow(a);
  return kDigestNone;
}

// A lane's run of findings of one tag into the tag's slot.
__device__ inline void digest_flush(const DigestArgs& a, uint64_t tag, uint64_t cnt, uint64_t rep) {
  if (!cnt) return;
  const uint64_t i = digest_slot(a, tag, true);
  if (i == kDigestNone) return;
  __hip_atomic_fetch_add(&a.table[i].count, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (digest_load(&a.table[i].rep) < rep)  // (the value only grows: a load that cannot win saves the atomic)
    __hip_atomic_fetch_max(&a.table[i].rep, rep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The sum of v over the wave, in lane 0.
__device__ inline uint64_t digest_wave_sum(uint64_t v) {
  for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
  return v;
}

// The string columns of `need` that are not resident (0: all are); a finding that lacks one is left out
// and the call answers KW_E_ARG.
__device__ inline uint32_t digest_lacks(const DigestArgs& a, uint32_t word) {
  const uint32_t lack = digest_need(digest_kind(KW_REASON(word))) & ~a.loaded;
  if (lack) __hip_atomic_fetch_or(&a.head->missing, lack, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return lack;
}

// The word walk of the verify and members kernels (digest.hpp digest_lane; the count kernel writes
// it out): a wave strides over units of kDigestRounds rounds, from `first` by `stride` rows, and a
// lane keeps its column.
struct Walk {
  PackGeom p;
  uint64_t rows, first, stride;  // (first: wave-uniform)
  uint32_t npol, c0, c1, grp, lane;
};
__device__ inline Walk walk_begin(const PackGeom& p, uint64_t rows, uint32_t npol, uint32_t c0, uint32_t c1) {
  const uint64_t unit = digest_unit_rows(p), wave = (uint64_t)blockIdx.x * kDigestWaves + (threadIdx.x >> 6);
  return Walk{p, rows, wave * unit, (uint64_t)kDigestWaves * gridDim.x * unit, npol, c0, c1, c0 / 64u + blockIdx.y, threadIdx.x & 63u};
}
// The lane's word of round t of the unit at row0; 0 (no finding) where it holds none. A kernel loads
// its unit's kDigestRounds words first, so that many loads are in flight before the first is used,
// and derives digest_lane again for the few words that are findings: through this struct the
// compiler kept every round's row and column live from the load to the use (members_walk_kernel: 126
// -> 144 VGPRs), through the kernel's own arguments it does not.
__device__ inline uint32_t walk_load(const Walk& w, const uint32_t* words, uint64_t row0, uint32_t t) {
  const DigestLane L = digest_lane(w.p, w.rows, w.c0, w.c1, w.grp, row0, t, w.lane);
  return L.on ? __builtin_nontemporal_load(words + L.row * w.npol + L.col) : 0u;
}

// A lane keeps one column for the whole launch, and a column's busy groups are few (a numeric key has a
// handful of values, a common capability many rows), so each lane holds kDigestHold runs of findings by
// tag in registers and only an evicted run, the one with the fewest findings, goes to the table: a busy
// group costs one add per eviction instead of one per finding (C4 1M: the count launch 21.3 -> 10.3 ms,
// profiles/r14_digest.txt).
constexpr uint32_t kDigestHold = 4;

__global__ void __launch_bounds__(256) digest_count_kernel(DigestArgs a, PackGeom p) {
  // (the walk of walk_begin / walk_load written out: through them this kernel spilled 64 SGPRs for
  // 46 and its launch took 2 to 7 % longer, profiles/r17_reports_refactor.txt)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, grp = a.c0 / 64u + blockIdx.y;
  const uint64_t unit = digest_unit_rows(p), stride = (uint64_t)kDigestWaves * gridDim.x * unit;
  uint64_t h_tag[kDigestHold], h_cnt[kDigestHold], h_rep[kDigestHold], n_find = 0;
#pragma unroll
  for (uint32_t k = 0; k < kDigestHold; ++k) h_tag[k] = h_cnt[k] = h_rep[k] = 0;
  for (uint64_t row0 = ((uint64_t)blockIdx.x * kDigestWaves + wave) * unit; row0 < a.cols.rows; row0 += stride) {  // wave-uniform
    // a range that has overflowed is cut and counted again: the rest of this launch is not needed
    if (__hip_atomic_load(&a.head->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;  // (one address: wave-uniform)
    uint32_t x[kDigestRounds];
#pragma unroll
    for (uint32_t t = 0; t < kDigestRounds; ++t) {
      const DigestLane L = digest_lane(p, a.cols.rows, a.c0, a.c1, grp, row0, t, lane);
      x[t] = L.on ? __builtin_nontemporal_load(a.words + L.row * a.npol + L.col) : 0u;  // (0: no finding)
    }
#pragma unroll
    for (uint32_t t = 0; t < kDigestRounds; ++t) {
      const uint32_t v = x[t];
      if (!digest_finding(v)) continue;
      ++n_find;
      const DigestLane L = digest_lane(p, a.cols.rows, a.c0, a.c1, grp, row0, t, lane);
      if (digest_wide(v)) {
        const uint64_t n = __hip_atomic_fetch_add(&a.head->nwide, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n < a.wide_cap) a.wide[n] = L.row * a.npol + L.col;
        continue;
      }
      if (digest_lacks(a, v)) continue;
      const uint64_t tag = digest_tag(digest_hash(L.col, digest_class(v), digest_key(a.cols, L.row, v)), a.hash_bits);
      const uint64_t rep = digest_rep(a.d2b ? a.d2b[L.row] : L.row, L.col);
      bool hit = false;
      uint32_t victim = 0;
      uint64_t least = ~0ull;
#pragma unroll
      for (uint32_t k = 0; k < kDigestHold; ++k) {
        if (!hit && h_tag[k] == tag) {
          ++h_cnt[k];
          h_rep[k] = rep > h_rep[k] ? rep : h_rep[k];
          hit = true;
        }
        if (h_cnt[k] < least) {  // (a free entry has count 0: taken first)
          least = h_cnt[k];
          victim = k;
        }
      }
      if (hit) continue;
#pragma unroll
      for (uint32_t k = 0; k < kDigestHold; ++k) {
        if (k != victim) continue;
        digest_flush(a, h_tag[k], h_cnt[k], h_rep[k]);
        h_tag[k] = tag;
        h_cnt[k] = 1;
        h_rep[k] = rep;
      }
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < kDigestHold; ++k) digest_flush(a, h_tag[k], h_cnt[k], h_rep[k]);
  n_find = digest_wave_sum(n_find);
  if (lane == 0u && n_find) __hip_atomic_fetch_add(&a.head->findings, n_find, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) digest_verify_kernel(DigestArgs a, PackGeom p) {
  const Walk w = walk_begin(p, a.cols.rows, a.npol, a.c0, a.c1);
  for (uint64_t row0 = w.first; row0 < w.rows; row0 += w.stride) {  // wave-uniform
    uint32_t x[kDigestRounds];
#pragma unroll
    for (uint32_t t = 0; t < kDigestRounds; ++t) x[t] = walk_load(w, a.words, row0, t);
#pragma unroll
    for (uint32_t t = 0; t < kDigestRounds; ++t) {
      const uint32_t v = x[t];
      if (!digest_finding(v) || digest_wide(v) || (digest_need(digest_kind(KW_REASON(v))) & ~a.loaded)) continue;
      const DigestLane L = digest_lane(p, a.cols.rows, a.c0, a.c1, w.grp, row0, t, w.lane);
      const DigestKey key = digest_key(a.cols, L.row, v);
      const uint64_t i = digest_slot(a, digest_tag(digest_hash(L.col, digest_class(v), key), a.hash_bits), false);
      bool same = false;
      if (i != kDigestNone) {
        const uint64_t rep = digest_load(&a.table[i].rep), rrow = digest_rep_row(rep);
        const uint32_t rcol = digest_rep_col(rep);
        if (rrow == (a.d2b ? a.d2b[L.row] : L.row) && rcol == L.col) continue;  // the representative itself
        if (rrow < a.cols.rows && rcol == L.col) {
          const uint64_t drow = a.b2d ? a.b2d[rrow] : rrow;
          const uint32_t rw = a.words[drow * a.npol + rcol];
          same = digest_finding(rw) && !digest_wide(rw) && digest_class(rw) == digest_class(v) &&
                 digest_same_key(key, digest_key(a.cols, drow, rw));
        }
      }
      if (same) continue;
      const uint64_t n = __hip_atomic_fetch_add(&a.head->nleft, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (n < a.left_cap) {
        DigestLeft e;
        e.pair = L.row * a.npol + L.col;
        e.word = v;
        e.pad = 0;
        a.left[n] = e;
      }
      if (i != kDigestNone) __hip_atomic_fetch_add(&a.table[i].count, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ void __launch_bounds__(256) digest_gather_kernel(DigestArgs a) {
  const uint64_t nt = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < a.nslots; i += nt) {
    const DigestSlot sl = a.table[i];
    if (sl.tag == 0u || sl.count == 0u) continue;
    const uint64_t row = digest_rep_row(sl.rep);
    const uint32_t col = digest_rep_col(sl.rep);
    if (row >= a.cols.rows || col >= a.npol) continue;  // (only a range the host discards holds such a slot)
    const uint64_t n = __hip_atomic_fetch_add(&a.head->nrec, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n >= a.rec_cap) continue;
    kw_digest_rec r;
    r.col = col;
    r.word = a.words[(a.b2d ? a.b2d[row] : row) * a.npol + col];
    r.first_row = row;
    r.count = sl.count;
    a.recs[n] = r;
  }
}

namespace {
// Workgroups for `items` at `per` a workgroup, while the device holds them at eight a CU: past that
// the threads stride. walk_wg_rows: `per` of the word walk, a wave a unit.
uint32_t walk_grid(uint64_t items, uint64_t per) {
  const uint64_t want = (items + per - 1u) / per, most = (uint64_t)std::max<uint32_t>(device_cus(), 1u) * 8u;
  return (uint32_t)std::min(want, most);
}
uint64_t walk_wg_rows(uint32_t npol) { return digest_unit_rows(pack_geom(npol)) * kDigestWaves; }

bool digest_grid(const DigestArgs& a, dim3* grid) {
  if (a.cols.rows == 0 || a.npol == 0 || a.c0 >= a.c1 || a.c1 > a.npol) return false;
  *grid = dim3(walk_grid(a.cols.rows, walk_wg_rows(a.npol)), (a.c1 - 1u) / 64u - a.c0 / 64u + 1u);
  return true;
}
}  // namespace

static hipError_t launch_digest_walk(void (*kernel)(DigestArgs, PackGeom), const DigestArgs& a, hipStream_t s) {
  dim3 grid;
  if (!digest_grid(a, &grid)) return hipSuccess;
  if (grid.y > 65535u || (a.nslots & (a.nslots - 1u)) || a.nslots == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, a, pack_geom(a.npol));
  return hipGetLastError();
}
hipError_t launch_digest_count(const DigestArgs& a, hipStream_t s) { return launch_digest_walk(digest_count_kernel, a, s); }
hipError_t launch_digest_verify(const DigestArgs& a, hipStream_t s) { return launch_digest_walk(digest_verify_kernel, a, s); }

hipError_t launch_digest_gather(const DigestArgs& a, hipStream_t s) {
  if (a.nslots == 0 || a.cols.rows == 0) return hipSuccess;
  hipLaunchKernelGGL(digest_gather_kernel, dim3(walk_grid(a.nslots, 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- the digest's drill-down (reports.hpp MembersArgs, members.hpp) ---------------------------------

__global__ void __launch_bounds__(256) members_check_kernel(MembersArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= a.nslots) return;
  const MemberSlot sl = a.table[i];
  if (sl.tag == 0u) return;
  if (sl.rep_row >= a.cols.rows || sl.col >= a.npol || a.words[sl.rep_row * a.npol + sl.col] != sl.word)
    __hip_atomic_store(&a.head->bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A lane's run of members of one group into the group's count.
__device__ inline void members_flush(const MembersArgs& a, uint32_t group, uint64_t n) {
  if (n) __hip_atomic_fetch_add(&a.counts[group], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) members_walk_kernel(MembersArgs a, PackGeom p) {
  const Walk w = walk_begin(p, a.cols.rows, a.npol, 0u, a.npol);
  const uint32_t lane = w.lane, mycol = 64u * w.grp + lane % p.w;
  // (a lane keeps a column for the whole launch: its mask of selected classes stays in a register)
  const uint64_t cmask = (lane / p.w < p.ipi && mycol < a.npol) ? a.colmask[mycol] : 0ull;
  if (!__ballot(cmask != 0ull)) return;  // wave-uniform: no named group lives in these columns
  uint32_t h_group = kMembersNone;
  uint64_t h_n = 0;
  for (uint64_t row0 = w.first; row0 < w.rows; row0 += w.stride) {  // wave-uniform
    uint32_t x[kDigestRounds], sel[kDigestRounds];
#pragma unroll
    for (uint32_t t = 0; t < kDigestRounds; ++t) x[t] = walk_load(w, a.words, row0, t);
    uint32_t mine = 0;  // this lane's members in the unit
#pragma unroll
    for (uint32_t t = 0; t < kDigestRounds; ++t) {
      const uint32_t v = x[t];
      sel[t] = kMembersNone;
      if (digest_finding(v) && !digest_wide(v) && ((cmask >> members_class_bit(digest_class(v))) & 1ull) &&
          !(digest_need(digest_kind(KW_REASON(v))) & ~a.loaded)) {
        const DigestLane L = digest_lane(p, a.cols.rows, 0u, a.npol, w.grp, row0, t, lane);
        sel[t] = members_find(a.table, a.nslots, a.cols, a.hash_bits, L.row, L.col, v);
      }
      mine += sel[t] != kMembersNone ? 1u : 0u;
    }
    if (!__ballot(mine != 0u)) continue;  // wave-uniform
    // one add per wave for the unit's members: an inclusive scan of the lanes' counts, the last lane
    // adds the total, every lane's members follow those of the lanes below it
    uint32_t upto = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)upto, d);
      if (lane >= d) upto += o;
    }
    uint64_t base = 0;
    if (lane == 63u) base = __hip_atomic_fetch_add(&a.head->nlist, (uint64_t)upto, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint64_t at = __shfl(base, 63) + (upto - mine);
#pragma unroll
    for (uint32_t t = 0; t < kDigestRounds; ++t) {
      const uint32_t group = sel[t];
      if (group == kMembersNone) continue;
      const DigestLane L = digest_lane(p, a.cols.rows, 0u, a.npol, w.grp, row0, t, lane);
      if (at < a.list_cap) {
        MemberEntry e;
        e.key = member_key(group, a.d2b ? a.d2b[L.row] : L.row);
        e.word = x[t];
        e.pad = 0;
        a.list[at] = e;
      }
      ++at;
      if (group == h_group) {
        ++h_n;
      } else {
        members_flush(a, h_group, h_n);
        h_group = group;
        h_n = 1;
      }
    }
  }
  members_flush(a, h_group, h_n);
}

hipError_t launch_members_check(const MembersArgs& a, hipStream_t s) {
  if (a.nslots == 0 || (a.nslots & (a.nslots - 1u)) || a.nslots > (1ull << 33)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(members_check_kernel, dim3((uint32_t)((a.nslots + 255u) / 256u)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_members_walk(const MembersArgs& a, hipStream_t s) {
  if (a.cols.rows == 0 || a.npol == 0) return hipSuccess;
  if (a.nslots == 0 || (a.nslots & (a.nslots - 1u))) return hipErrorInvalidValue;
  const uint32_t gy = packed_groups(a.npol);
  if (gy > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(members_walk_kernel, dim3(walk_grid(a.cols.rows, walk_wg_rows(a.npol)), gy), dim3(256), 0, s, a, pack_geom(a.npol));
  return hipGetLastError();
}

// ---- the messages of chosen findings (reports.hpp MessagesArgs, messages.hpp) -----------------------

__global__ void __launch_bounds__(256) messages_len_kernel(MessagesArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t row = a.drow[i];
  const uint32_t col = a.col[i];
  uint32_t word = 0, st = MSG_TEXT;
  MsgPlan P;
  P.npc = 0;
  P.len = 0;
  if (row < a.cols.c.rows && col < a.npol) {  // (the host checked both: nothing is read outside the pass)
    word = a.words[row * a.npol + col];
    st = message_pieces(a.cols, msg_settings(a.settings), row, col, word, &P);
  }
  a.len[i] = st == MSG_TEXT ? P.len : 0u;
  a.mark[i] = st == MSG_HOST ? 1u : 0u;
  if (a.out_words) a.out_words[i] = word;
  if (st == MSG_MISSING) __hip_atomic_store(&a.head->missing, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sums: a workgroup a tile of kMsgScanTile lengths, its total into sums[tile].
__global__ void __launch_bounds__(kMsgScanThreads) messages_sums_kernel(MessagesArgs a) {
  __shared__ uint64_t wave_sum[kMsgScanThreads / 64u];
  const uint32_t i = blockIdx.x * kMsgScanTile + 4u * threadIdx.x;
  uint64_t mine = 0, total;
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j) mine += i + j < a.n ? a.len[i + j] : 0u;
  (void)block_scan<uint64_t, kMsgScanThreads>(mine, wave_sum, &total);
  if (threadIdx.x == 0u) a.sums[blockIdx.x] = total;
}

// bases: one workgroup turns the tiles' totals into their bases (base + the totals before), in
// place, and writes the round's end into off[n].
__global__ void __launch_bounds__(kMsgScanThreads) messages_bases_kernel(MessagesArgs a) {
  __shared__ uint64_t wave_sum[kMsgScanThreads / 64u];
  const uint32_t nt = (a.n + kMsgScanTile - 1u) / kMsgScanTile;
  const uint64_t carry = scan_bases<uint64_t, kMsgScanThreads, kMsgScanTile / kMsgScanThreads>(a.sums, nt, a.base, wave_sum);
  if (threadIdx.x == 0u) a.off[a.n] = carry;
}

// scan: a workgroup a tile again, its offsets from the tile's base.
__global__ void __launch_bounds__(kMsgScanThreads) messages_scan_kernel(MessagesArgs a) {
  __shared__ uint64_t wave_sum[kMsgScanThreads / 64u];
  const uint32_t i = blockIdx.x * kMsgScanTile + 4u * threadIdx.x;
  uint32_t l[4];
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j) l[j] = i + j < a.n ? a.len[i + j] : 0u;
  uint64_t total;
  uint64_t at = a.sums[blockIdx.x] + block_scan<uint64_t, kMsgScanThreads>((uint64_t)l[0] + l[1] + l[2] + l[3], wave_sum, &total);
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j) {
    if (i + j < a.n) a.off[i + j] = at;
    at += l[j];
  }
}

extern __shared__ uint4 messages_window[];

// What the write kernels of the messages, the responses and the patches share: the window [wb, wb +
// window) of LDS, filled by the lanes, leaves for the wave's byte range [rb, re) of the text: aligned
// 16-byte stores, the range's unaligned head and tail in single bytes, nothing outside the range.
__device__ inline void window_store(uint8_t* text, uint64_t text_base, const uint8_t* lds, uint64_t wb, uint32_t window, uint64_t rb,
                                    uint64_t re, uint32_t lane) {
  __syncthreads();  // one wave: the LDS writes are done before any lane reads the window
  const uint64_t lo = wb > rb ? wb : rb, hi = wb + window < re ? wb + window : re;
  uint64_t body, tail;
  msg_chunks(lo, hi, &body, &tail);
  for (uint64_t g = lo + lane; g < body; g += 64u) text[g - text_base] = lds[g - wb];
  for (uint64_t g = body + 16u * lane; g < tail; g += 16u * 64u) *(uint4*)(text + (g - text_base)) = *(const uint4*)(lds + (g - wb));
  for (uint64_t g = tail + lane; g < hi; g += 64u) text[g - text_base] = lds[g - wb];
  __syncthreads();  // the window is read before the next one is filled
}
// One lane adds the wave's windows and its items that spanned more than one to the call's counters.
template <typename Head>
__device__ inline void window_counts(Head* head, uint64_t nwin, uint64_t span) {
  __hip_atomic_fetch_add(&head->windows, nwin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (span) __hip_atomic_fetch_add(&head->spanning, span, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(64) messages_write_kernel(MessagesArgs a) {
  const uint32_t lane = threadIdx.x, i0 = blockIdx.x * kMsgWaveItems, i = i0 + lane;
  const uint32_t i1 = i0 + kMsgWaveItems < a.n ? i0 + kMsgWaveItems : a.n;
  const uint64_t rb = a.off[i0], re = a.off[i1];  // the wave's byte range
  if (re <= rb) return;                           // uniform: 64 empty messages
  MsgPlan P;
  P.npc = 0;
  P.len = 0;
  uint64_t mb = rb;
  if (i < a.n) {
    mb = a.off[i];
    const uint64_t row = a.drow[i];
    const uint32_t col = a.col[i];
    if (row < a.cols.c.rows && col < a.npol &&
        message_pieces(a.cols, msg_settings(a.settings), row, col, a.words[row * a.npol + col], &P) != MSG_TEXT) {
      P.npc = 0;
      P.len = 0;
    }
    if ((uint64_t)P.len != a.off[i + 1] - mb) {  // (not the message the lengths were counted from: nothing is copied)
      P.npc = 0;
      P.len = 0;
    }
  }
  uint8_t* lds = (uint8_t*)messages_window;
  const uint64_t w0 = rb & ~(uint64_t)15u;
  uint64_t nwin = 0;
  for (uint64_t wb = w0; wb < re; wb += a.window, ++nwin) {  // uniform
    uint32_t skip, at, n;
    msg_clip(mb, P.len, wb, a.window, &skip, &at, &n);
    if (n) msg_copy_window(P, skip, n, lds + at);
    window_store(a.text, a.text_base, lds, wb, a.window, rb, re, lane);
  }
  const uint64_t span = __popcll(__ballot(msg_windows_of(mb, P.len, w0, a.window) > 1u));
  if (lane == 0u) window_counts(a.head, nwin, span);
}

hipError_t launch_messages_len(const MessagesArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(messages_len_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_messages_scan(const MessagesArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  const uint32_t tiles = (a.n + kMsgScanTile - 1u) / kMsgScanTile;
  hipLaunchKernelGGL(messages_sums_kernel, dim3(tiles), dim3(kMsgScanThreads), 0, s, a);
  hipLaunchKernelGGL(messages_bases_kernel, dim3(1), dim3(kMsgScanThreads), 0, s, a);
  hipLaunchKernelGGL(messages_scan_kernel, dim3(tiles), dim3(kMsgScanThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_messages_write(const MessagesArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  if (a.window < kMsgMinWindow || a.window > kMsgMaxWindow || (a.window & 15u) || (a.text_base & 15u)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(messages_write_kernel, dim3((a.n + kMsgWaveItems - 1u) / kMsgWaveItems), dim3(64), a.window, s, a);
  return hipGetLastError();
}

// ---- the response bodies of chosen pairs (reports.hpp ResponsesArgs, responses.hpp) -----------------

__device__ inline RspCtx responses_ctx(const ResponsesArgs& a) {
  RspCtx X;
  X.C = a.cols;
  X.uid = a.uid;
  X.S = rsp_settings(a.settings);
  X.words = a.words;
  X.npol = a.npol;
  return X;
}

__global__ void __launch_bounds__(256) responses_len_kernel(ResponsesArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t row = a.drow[i];
  const uint32_t col = a.col[i];
  uint32_t word = 0, st = RSP_TEXT, len = 0, nesc = 0;
  if (row < a.cols.c.rows && col < a.npol) {  // (the host checked both: nothing is read outside the pass)
    const RspCtx X = responses_ctx(a);
    word = a.words[row * a.npol + col];
    RspItem it;
    st = col < X.S.ncols ? rsp_item(X.S, col, word, &it) : (uint32_t)RSP_HOST;
    if (st == RSP_TEXT) st = rsp_measure(X, row, col, word, it, &len, &nesc);
  }
  a.len[i] = st == RSP_TEXT ? len : 0u;
  a.mark[i] = st == RSP_HOST ? 1u : 0u;
  if (a.out_words) a.out_words[i] = word;
  if (st == RSP_MISSING) __hip_atomic_store(&a.head->missing, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (st == RSP_TEXT && nesc) __hip_atomic_fetch_add(&a.head->escaped, (uint64_t)nesc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

extern __shared__ uint4 responses_window[];

__global__ void __launch_bounds__(64) responses_write_kernel(ResponsesArgs a) {
  const uint32_t lane = threadIdx.x, i0 = blockIdx.x * kMsgWaveItems, i = i0 + lane;
  const uint32_t i1 = i0 + kMsgWaveItems < a.n ? i0 + kMsgWaveItems : a.n;
  const uint64_t rb = a.off[i0], re = a.off[i1];  // the wave's byte range
  if (re <= rb) return;                           // uniform: 64 empty responses
  const RspCtx X = responses_ctx(a);
  RspItem it;
  it.form = RF_SHORT;
  it.nparts = 0;
  it.mask = 0;
  uint64_t mb = rb, row = 0;
  uint32_t col = 0, word = 0, len = 0;
  if (i < a.n) {
    mb = a.off[i];
    row = a.drow[i];
    col = a.col[i];
    // the length the offsets were scanned from: an item left to the host has none, and nothing is
    // written past it whatever the parts give
    len = (uint32_t)(a.off[i + 1] - mb);
    if (len != a.len[i] || row >= a.cols.c.rows || col >= a.npol || col >= X.S.ncols) len = 0;
    if (len) {
      word = a.words[row * a.npol + col];
      if (rsp_item(X.S, col, word, &it) != RSP_TEXT) len = 0;
    }
  }
  uint8_t* lds = (uint8_t*)responses_window;
  const uint64_t w0 = rb & ~(uint64_t)15u;
  uint64_t nwin = 0;
  for (uint64_t wb = w0; wb < re; wb += a.window, ++nwin) {  // uniform
    uint32_t skip, at, n;
    msg_clip(mb, len, wb, a.window, &skip, &at, &n);
    if (n) rsp_render_window(X, row, col, word, it, skip, n, lds + at);
    window_store(a.text, a.text_base, lds, wb, a.window, rb, re, lane);
  }
  const uint64_t span = __popcll(__ballot(msg_windows_of(mb, len, w0, a.window) > 1u));
  if (lane == 0u) window_counts(a.head, nwin, span);
}

hipError_t launch_responses_len(const ResponsesArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(responses_len_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_responses_write(const ResponsesArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  if (a.window < kMsgMinWindow || a.window > kMsgMaxWindow || (a.window & 15u) || (a.text_base & 15u)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(responses_write_kernel, dim3((a.n + kMsgWaveItems - 1u) / kMsgWaveItems), dim3(64), a.window, s, a);
  return hipGetLastError();
}

// ---- the JSONPatch of accepted mutations (reports.hpp PatchesArgs, patches.hpp) ------------------------

__device__ inline PatchCtx patches_ctx(const PatchesArgs& pa) {
  PatchCtx X;
  X.C = pa.c;
  X.S = patch_settings(pa.r.settings);
  return X;
}

__global__ void __launch_bounds__(256) patches_len_kernel(PatchesArgs pa) {
  const ResponsesArgs& a = pa.r;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t row = a.drow[i];
  const uint32_t col = a.col[i];
  uint32_t word = 0, st = PATCH_HOST, len = 0;
  if (row < pa.c.rows && col < a.npol) {  // (the host checked both: nothing is read outside the pass)
    const PatchCtx X = patches_ctx(pa);
    word = a.words[row * a.npol + col];
    if (col < X.S.ncols) st = patch_length(X, row, col, word, pa.form, &len);
  }
  a.len[i] = st == PATCH_TEXT ? len : 0u;
  a.mark[i] = st == PATCH_HOST ? 1u : 0u;
  if (a.out_words) a.out_words[i] = word;
  if (st == PATCH_MISSING) __hip_atomic_store(&a.head->missing, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

extern __shared__ uint4 patches_window[];

__global__ void __launch_bounds__(64) patches_write_kernel(PatchesArgs pa) {
  const ResponsesArgs& a = pa.r;
  const uint32_t lane = threadIdx.x, i0 = blockIdx.x * kMsgWaveItems, i = i0 + lane;
  const uint32_t i1 = i0 + kMsgWaveItems < a.n ? i0 + kMsgWaveItems : a.n;
  const uint64_t rb = a.off[i0], re = a.off[i1];  // the wave's byte range
  if (re <= rb) return;                           // uniform: 64 items without text
  const PatchCtx X = patches_ctx(pa);
  const bool response = pa.form == (uint32_t)KW_PATCH_RESPONSE;
  PatchEnvelope env;
  env.uid = nullptr;
  env.un = env.ue = env.head = 0;
  uint64_t mb = rb, row = 0;
  uint32_t col = 0, len = 0, ops = 0;
  if (i < a.n) {
    mb = a.off[i];
    row = a.drow[i];
    col = a.col[i];
    // the length the offsets were scanned from: an item left to the host has none, and nothing is
    // written past it whatever the walk gives
    len = (uint32_t)(a.off[i + 1] - mb);
    if (len != a.len[i] || row >= pa.c.rows || col >= a.npol || col >= X.S.ncols) len = 0;
    if (len && patch_item(X, row, col, a.words[row * a.npol + col], pa.form) != PATCH_TEXT) len = 0;
    if (len) {
      ops = patch_measure(X, row, col);
      if (response) env = patch_envelope(X, row);
      if ((response ? patch_response_len(env, ops) : ops) != len) len = 0;
    }
  }
  uint8_t* lds = (uint8_t*)patches_window;
  uint8_t* raw = lds + a.window;  // the raw ops bytes under a lane's base64 quads (patches_raw_bytes)
  const uint64_t w0 = rb & ~(uint64_t)15u;
  uint64_t nwin = 0;
  for (uint64_t wb = w0; wb < re; wb += a.window, ++nwin) {  // uniform
    uint32_t skip, at, n;
    msg_clip(mb, len, wb, a.window, &skip, &at, &n);
    if (n) {
      // lane k's part of the window starts after lane k - 1's: 3 x (at / 4) + 8 x lane leaves every
      // lane patch_raw_need(n) bytes of its own
      if (response) patch_response_window(X, row, col, env, ops, skip, n, lds + at, raw + 3u * (at / 4u) + 8u * lane);
      else patch_render_window(X, row, col, skip, n, lds + at);
    }
    window_store(a.text, a.text_base, lds, wb, a.window, rb, re, lane);
  }
  const uint64_t span = __popcll(__ballot(msg_windows_of(mb, len, w0, a.window) > 1u));
  if (lane == 0u) window_counts(a.head, nwin, span);
}

// The LDS of the write kernel: the window and the raw bytes beside it.
static uint32_t patches_raw_bytes(uint32_t window) { return (3u * (window / 4u) + 8u * 64u + 16u + 15u) & ~15u; }

hipError_t launch_patches_len(const PatchesArgs& pa, hipStream_t s) {
  if (pa.r.n == 0) return hipSuccess;
  hipLaunchKernelGGL(patches_len_kernel, dim3((pa.r.n + 255u) / 256u), dim3(256), 0, s, pa);
  return hipGetLastError();
}

hipError_t launch_patches_write(const PatchesArgs& pa, hipStream_t s) {
  const ResponsesArgs& a = pa.r;
  if (a.n == 0) return hipSuccess;
  if (a.window < kMsgMinWindow || a.window > kMsgMaxWindow || (a.window & 15u) || (a.text_base & 15u)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(patches_write_kernel, dim3((a.n + kMsgWaveItems - 1u) / kMsgWaveItems), dim3(64),
                     a.window + patches_raw_bytes(a.window), s, pa);
  return hipGetLastError();
}

}  // namespace kw
