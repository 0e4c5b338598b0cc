// groups.hpp — launch interface of the wide path's combine kernel (groups.hip), which writes the
// columns of wide policy groups and split policies from their members' verdict words.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "slots.hpp"

namespace kw {

// Wide policy groups (expr.hpp: more than 64 members, or a value stack deeper than 64): the
// members ran as a separate all-pairs pass into `member_words` [row][nmw]; the combine kernel runs
// each group's jump code per row over their results. One record per wide group column of the pass.
struct WideGroupArgs {
  uint32_t prog_off, prog_len;  // jump code in `progs`
  uint32_t col;                 // all-pairs: the group's output column; rows mode: its column id
  uint32_t nmem, midx_off;      // member slot s -> member_words column midx[midx_off + s]
  uint32_t okw, rejb;           // the group's accepted / rejected verdict words (reason GROUP, ARG wide)
  uint32_t cause_off, cause_words;  // its cause bitset in the per-row side data
  uint32_t errw;                // script programs: the evaluation-error verdict word (reason GROUP_EXPR)
  uint32_t kind;                // 0 jump code (run_wide_prog), 1 script bytecode (run_script_prog),
                                // 2 / 3 a split safe-labels / psp-capabilities policy (combine_parts)
  uint32_t mutw;                // split psp-capabilities: the mutated verdict word
};

constexpr uint32_t kSplitMember = 0x80000000u;  // a group's midx entry naming a split member's record

// A split policy's word from its parts' words (env.cpp split_policy): the first part that rejects
// (safe-labels: a mandatory index offset by the part's start), else — psp-capabilities, whose later
// parts validate nothing — mutated when any part mutated, else accepted. part(s): part s's word.
template <class Part>
KW_HD inline uint32_t combine_parts(const WideGroupArgs& g, const uint32_t* part_off, Part part) {
  bool mutated = false;
  for (uint32_t s = 0; s < g.nmem; ++s) {
    const uint32_t x = part(s);
    if (!(x & KW_V_ALLOWED)) {
      uint32_t reason = KW_REASON(x), arg = KW_ARG(x);
      if (reason == KW_R_LABEL_MANDATORY && arg != kArgWide) arg += part_off[s];
      return g.rejb | vword(reason, arg);
    }
    if (x & KW_V_MUTATED) mutated = true;
  }
  return mutated ? g.mutw : g.okw;
}
struct WideGroupPass {
  const WideGroupArgs* groups;
  uint32_t ngroups;
  const uint8_t* progs;
  const uint32_t* midx;
  const uint32_t* member_words;  // [row][nmw]
  uint32_t nmw;
  uint32_t* out;                 // the pass's verdict words
  uint32_t npol;                 // all-pairs stride; rows mode: 1
  const uint32_t* rowcol;        // rows mode: the row's column id (== WideGroupArgs::col), nullptr = all pairs
  uint64_t* causes;              // [row][cause_stride] u64
  uint32_t cause_stride;
  uint64_t* stack;               // scratch: stack_words u64 per thread of the grid
  uint32_t stack_words;
  uint64_t nrows;
};
hipError_t launch_wide_groups(const WideGroupPass& w, uint32_t grid, hipStream_t s);

}  // namespace kw
