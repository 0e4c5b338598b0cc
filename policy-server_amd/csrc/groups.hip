// groups.hip — the combine kernel of the wide path (groups.hpp): the columns of wide policy groups
// and split policies from their members' verdict words, the group programs run by groupvm.hpp. A
// translation unit of its own: it uses none of the hot path's device code (kernels.hip), so a
// change of the script VM does not recompile the tile kernel's instantiations, nor the reverse.
#include <hip/hip_runtime.h>

#include "../../include/kwgpu.h"
#include "groups.hpp"
#include "groupvm.hpp"

namespace kw {

// ------------------------------------------------------------------------------------------
// Wide policy groups: the members' verdict words of a separate pass -> each group's jump code per
// row (groupvm.hpp run_wide_prog), its value stack in this thread's scratch words and its causes in
// the per-row side data. A row the main pass answered with the bypass word keeps it.
// ------------------------------------------------------------------------------------------
constexpr int kWideThreads = 256;

__global__ void __launch_bounds__(kWideThreads) wide_groups_kernel(WideGroupPass w) {
  const uint64_t nthreads = (uint64_t)gridDim.x * kWideThreads;
  const uint64_t gtid = (uint64_t)blockIdx.x * kWideThreads + threadIdx.x;
  uint64_t* stack = w.stack + gtid * w.stack_words;
  const uint64_t pairs = w.nrows * w.ngroups;
  for (uint64_t q = gtid; q < pairs; q += nthreads) {
    const uint64_t r = q / w.ngroups;
    const WideGroupArgs& g = w.groups[q - r * w.ngroups];
    uint32_t* dst;
    if (w.rowcol) {
      if (w.rowcol[r] != g.col) continue;
      dst = w.out + r;
    } else {
      dst = w.out + r * w.npol + g.col;
    }
    if (*dst == kBypassWord) continue;
    uint64_t* cz = w.causes + r * w.cause_stride + g.cause_off;
    for (uint32_t k = 0; k < g.cause_words; ++k) cz[k] = 0;
    const uint32_t* mw = w.member_words + r * w.nmw;
    const uint32_t* midx = w.midx + g.midx_off;
    auto ok = [&](uint32_t s) {
      const uint32_t c = midx[s];
      uint32_t x;
      if (c & kSplitMember) {  // a split member: its word from its parts' words
        const WideGroupArgs& a = w.groups[w.ngroups + (c & ~kSplitMember)];
        const uint32_t* am = w.midx + a.midx_off;
        x = combine_parts(a, (const uint32_t*)(w.progs + a.prog_off), [&](uint32_t t) { return mw[am[t]]; });
      } else {
        x = mw[c];
      }
      return (x & KW_V_ALLOWED) && !(x & KW_V_MUTATED);
    };
    auto cause = [&](uint32_t s) { cz[s >> 6] |= 1ull << (s & 63u); };
    // a group of at most 15 members carries its causes in ARG, as column_word's forms do
    // (a group without members has no cause words: cz then points past its own range)
    auto rej = [&]() {
      const uint32_t c0 = g.cause_words ? (uint32_t)cz[0] : 0u;
      return g.nmem <= 15 ? (g.rejb & 0xffffu) | (c0 << 16) : g.rejb;
    };
    if (g.kind == 1) {  // script bytecode: true, false or an evaluation error
      const int v = run_script_prog(w.progs + g.prog_off, stack, ok, cause);
      *dst = v == 1 ? g.okw : v == 0 ? rej() : g.errw;
      continue;
    }
    if (g.kind >= 2) {  // a split plain policy: its parts' words
      *dst = combine_parts(g, (const uint32_t*)(w.progs + g.prog_off), [&](uint32_t s) { return mw[midx[s]]; });
      continue;
    }
    const bool v = run_wide_prog(w.progs + g.prog_off, g.prog_len, stack, ok, cause);
    *dst = v ? g.okw : rej();
  }
}

hipError_t launch_wide_groups(const WideGroupPass& w, uint32_t grid, hipStream_t s) {
  if (w.nrows == 0 || w.ngroups == 0) return hipSuccess;
  hipLaunchKernelGGL(wide_groups_kernel, dim3(grid), dim3(kWideThreads), 0, s, w);
  return hipGetLastError();
}

}  // namespace kw
