// knobs.cpp — the one getenv of libkwgpu.so, the parsers of the kKnobs rows and the plan cache's
// key over them (knobs.hpp).
#include "knobs.hpp"

#include <cstdlib>

namespace kw {
namespace knob_detail {

const char* env(const KnobRow& r) { return getenv(r.name); }

bool parse_bool(const KnobRow& r) {
  const char* v = env(r);
  switch (r.kind) {
    case KnobKind::On: return !(v && atoi(v) == 0);
    case KnobKind::Present: return v != nullptr;
    default: return v && atoi(v) != 0;
  }
}

int parse_int(const KnobRow& r) {
  const char* v = env(r);
  if (!v) return r.def;
  const int x = atoi(v);
  if (x < r.lo) return r.clamp ? r.lo : r.def;
  if (x > r.hi) return r.clamp ? r.hi : r.def;
  return x;
}

double parse_double(const KnobRow& r) {
  const char* v = env(r);
  return v ? atof(v) : r.dflt;
}

}  // namespace knob_detail

uint64_t kw_knob_hash() {
  uint64_t h = 1469598103934665603ull;
  for (const KnobRow& r : kKnobs) {
    if (!r.plans) continue;
    const char* v = knob_detail::env(r);
    h = (h ^ (v ? 0x100u : 0x200u)) * 1099511628211ull;
    for (const char* c = v; c && *c; ++c) h = (h ^ (uint8_t)*c) * 1099511628211ull;
  }
  return h;
}

}  // namespace kw
