// knobs.hpp — every KW_* run-time setting of libkwgpu.so: one table (kKnobs), typed accessors keyed
// by the Knob enum. Nothing else in the library reads the environment (knobs.cpp does).
//
// Lifetime: a latched setting is parsed at its first read and keeps that value for the process; a
// live one is parsed at every read (tests switch those between passes).
// Planning: a row flagged `plans` is part of the plan cache's key (kw_knob_hash). A translation
// unit that plans a pass (plan.cpp, slotplan.cpp, expr.cpp) defines KW_PLANNING_TU before this
// header and then sees PlanKnobs only, whose every read static_asserts that flag: such a source
// cannot read a setting the key leaves out. (The rule binds the sources that opt in; a new
// planning source has to define KW_PLANNING_TU too.)
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>

namespace kw {

enum Knob : int {
  KW_STREAM_POOL, KW_HOST_THREADS, KW_L2_PREFETCH, KW_KV_GLOBAL, KW_NO_MPACK,
  KW_BULK_DEBUG, KW_BULK_SAMPLE, KW_BULK_PACK, KW_BULK_CHUNK, KW_BULK_RAMP, KW_BULK_DIRECT, KW_BULK_DEPTH,
  KW_SCHED, KW_SCHED_TAIL, KW_SPLIT, KW_GROUP_FORM, KW_POISON_VERDICTS, KW_FLATTEN_THREADS,
  KW_SLOT_ROWS, KW_HEAVY_ROWS, KW_HEAVY_CTR, KW_GLOBAL_TABLES, KW_TILE_SPLIT, KW_ROUND_SPLIT,
  KW_TILE_QUANTILE, KW_TILE_DEBUG, KW_TILE_CUT, KW_OUTCOME_TABLE, KW_TILE_GENERIC,
  KW_DIGEST_TABLE, KW_DIGEST_HASH_BITS, KW_MESSAGES_CHUNK, KW_MESSAGES_WINDOW,
  KW_NKNOBS
};

enum class KnobKind : uint8_t {
  On,       // bool: on unless the value parses to 0
  Off,      // bool: off unless the value parses to non-zero
  Present,  // bool: on when the variable exists at all (even "=0")
  Int,      // atoi; outside [lo, hi] it clamps (clamp) or counts as unset; unset: def
  Double,   // atof; unset: dflt
  Str       // the value itself; unset: ""
};

struct KnobRow {
  const char* name;
  KnobKind kind;
  bool latched;  // parsed once at first read, else at every read
  bool plans;    // read while a pass is planned: part of the plan cache's key
  int def, lo, hi;
  bool clamp;
  double dflt;
  const char* what;
};

constexpr KnobRow knob_flag(const char* name, KnobKind k, bool latched, bool plans, const char* what) {
  return {name, k, latched, plans, 0, 0, 0, false, 0.0, what};
}
constexpr KnobRow knob_int(const char* name, bool latched, bool plans, int def, int lo, int hi, bool clamp, const char* what) {
  return {name, KnobKind::Int, latched, plans, def, lo, hi, clamp, 0.0, what};
}
constexpr KnobRow knob_real(const char* name, bool plans, double dflt, const char* what) {
  return {name, KnobKind::Double, false, plans, 0, 0, 0, false, dflt, what};
}

constexpr bool kLatched = true, kLive = false, kPlans = true, kNoPlan = false, kClamp = true, kElseUnset = false;

// In Knob order (checked below).
constexpr KnobRow kKnobs[KW_NKNOBS] = {
    knob_flag("KW_STREAM_POOL", KnobKind::On, kLatched, kNoPlan, "reuse streams and events per device"),
    knob_int("KW_HOST_THREADS", kLatched, kNoPlan, 0, 1, INT_MAX, kClamp, "host worker threads (unset: the hardware's, at most 16)"),
    knob_flag("KW_L2_PREFETCH", KnobKind::Off, kLatched, kPlans, "run the next-tile L2 prefetch (kernels built with KW_PREFETCH)"),
    knob_flag("KW_KV_GLOBAL", KnobKind::Off, kLatched, kPlans, "label-value DFAs read from global memory, not staged"),
    knob_flag("KW_NO_MPACK", KnobKind::Present, kLatched, kPlans, "slot plans without mandatory-field batching"),
    knob_flag("KW_BULK_DEBUG", KnobKind::Off, kLatched, kNoPlan, "print host stage times of planning and the bulk path"),
    knob_flag("KW_BULK_SAMPLE", KnobKind::On, kLatched, kNoPlan, "bulk path: tile capacities from ~2048 sampled tiles"),
    knob_flag("KW_BULK_PACK", KnobKind::On, kLatched, kNoPlan, "bulk path: packed chunks through their own ring"),
    knob_int("KW_BULK_CHUNK", kLatched, kNoPlan, 262144, 1, INT_MAX, kClamp, "bulk path: rows per chunk"),
    knob_flag("KW_BULK_RAMP", KnobKind::On, kLatched, kNoPlan, "bulk path: small first and last chunks"),
    knob_flag("KW_BULK_DIRECT", KnobKind::On, kLatched, kNoPlan, "bulk path: read back straight into pinned output"),
    knob_int("KW_BULK_DEPTH", kLatched, kNoPlan, -1, 0, INT_MAX, kClamp, "bulk path: chunks in flight (0: unbounded; unset: 2 or 3)"),
    knob_flag("KW_SCHED", KnobKind::Str, kLive, kPlans, "static / dynamic: force one tile schedule"),
    knob_int("KW_SCHED_TAIL", kLive, kPlans, -1, 0, INT_MAX, kElseUnset, "rounds a strided launch draws from the counters at its end (0: none; unset: chosen per launch)"),
    knob_int("KW_SPLIT", kLive, kPlans, -1, INT_MIN, INT_MAX, kClamp, "0: never split light / heavy rows, 1: whenever both exist"),
    knob_flag("KW_GROUP_FORM", KnobKind::Str, kLive, kPlans, "script: compile every group expression as a script"),
    knob_flag("KW_POISON_VERDICTS", KnobKind::Off, kLive, kPlans, "fill the verdict words with a sentinel before a pass"),
    knob_int("KW_FLATTEN_THREADS", kLive, kNoPlan, 0, 1, INT_MAX, kClamp, "JSON flatten threads (unset: the hardware's, at most 16)"),
    knob_int("KW_SLOT_ROWS", kLive, kPlans, 0, 8, 255, kElseUnset, "force the tile height"),
    knob_int("KW_HEAVY_ROWS", kLive, kPlans, 0, 8, 255, kElseUnset, "force the heavy region's tile height"),
    knob_int("KW_HEAVY_CTR", kLive, kPlans, 5, 1, INT_MAX, kElseUnset, "containers above which a request is heavy"),
    knob_flag("KW_GLOBAL_TABLES", KnobKind::Off, kLive, kPlans, "classifier tables read from global memory"),
    knob_real("KW_TILE_SPLIT", kPlans, 0.02, "share of tiles a capacity choice may split"),
    knob_real("KW_ROUND_SPLIT", kPlans, 0.02, "share of a taller tile's tiles that may need a second P1 round"),
    knob_real("KW_TILE_QUANTILE", kPlans, 0.0, "force the capacity quantile (unset: chosen per batch)"),
    knob_int("KW_TILE_DEBUG", kLive, kPlans, 0, INT_MIN, INT_MAX, kClamp, "kernel phase ablation bits; 256: print the plan"),
    knob_flag("KW_TILE_CUT", KnobKind::On, kLive, kPlans, "end each tile at the row of least estimated cost per row (0: fixed height)"),
    knob_int("KW_OUTCOME_TABLE", kLive, kNoPlan, 64 << 20, 1, INT_MAX, kClamp, "kw_batch_outcomes: bytes of the device table (more groups are counted in ranges)"),
    knob_flag("KW_TILE_GENERIC", KnobKind::Off, kLive, kPlans, "every tile launch on the generic kernel, none on a production-shape one"),
    knob_int("KW_DIGEST_TABLE", kLive, kNoPlan, 64 << 20, 1, INT_MAX, kClamp, "kw_batch_digest: bytes of the device hash table (more groups are reduced in column ranges)"),
    knob_int("KW_DIGEST_HASH_BITS", kLive, kNoPlan, 64, 0, 64, kClamp, "kw_batch_digest: low bits of the key hash that are kept (tests: fewer make every probe collide)"),
    knob_int("KW_MESSAGES_CHUNK", kLive, kNoPlan, 1 << 20, 1, 1 << 24, kClamp, "kw_batch_messages: items of one round (the device scratch is sized by it)"),
    knob_int("KW_MESSAGES_WINDOW", kLive, kNoPlan, 4096, 256, 32768, kClamp, "kw_batch_messages: bytes of the LDS window a wave writes its text through (a multiple of 16)"),
};

constexpr bool knob_name_is(const char* a, const char* b) {
  while (*a && *a == *b) ++a, ++b;
  return *a == *b;
}
#define KW_KNOB_ROW(K) static_assert(knob_name_is(kKnobs[K].name, #K), "kKnobs is not in Knob order")
KW_KNOB_ROW(KW_STREAM_POOL); KW_KNOB_ROW(KW_HOST_THREADS); KW_KNOB_ROW(KW_L2_PREFETCH); KW_KNOB_ROW(KW_KV_GLOBAL);
KW_KNOB_ROW(KW_NO_MPACK); KW_KNOB_ROW(KW_BULK_DEBUG); KW_KNOB_ROW(KW_BULK_SAMPLE); KW_KNOB_ROW(KW_BULK_PACK);
KW_KNOB_ROW(KW_BULK_CHUNK); KW_KNOB_ROW(KW_BULK_RAMP); KW_KNOB_ROW(KW_BULK_DIRECT); KW_KNOB_ROW(KW_BULK_DEPTH);
KW_KNOB_ROW(KW_SCHED); KW_KNOB_ROW(KW_SCHED_TAIL); KW_KNOB_ROW(KW_SPLIT); KW_KNOB_ROW(KW_GROUP_FORM); KW_KNOB_ROW(KW_POISON_VERDICTS);
KW_KNOB_ROW(KW_FLATTEN_THREADS); KW_KNOB_ROW(KW_SLOT_ROWS); KW_KNOB_ROW(KW_HEAVY_ROWS); KW_KNOB_ROW(KW_HEAVY_CTR);
KW_KNOB_ROW(KW_GLOBAL_TABLES); KW_KNOB_ROW(KW_TILE_SPLIT); KW_KNOB_ROW(KW_ROUND_SPLIT); KW_KNOB_ROW(KW_TILE_QUANTILE);
KW_KNOB_ROW(KW_TILE_DEBUG); KW_KNOB_ROW(KW_TILE_CUT); KW_KNOB_ROW(KW_OUTCOME_TABLE); KW_KNOB_ROW(KW_TILE_GENERIC);
KW_KNOB_ROW(KW_DIGEST_TABLE); KW_KNOB_ROW(KW_DIGEST_HASH_BITS); KW_KNOB_ROW(KW_MESSAGES_CHUNK); KW_KNOB_ROW(KW_MESSAGES_WINDOW);
#undef KW_KNOB_ROW

// The plan cache's key for the KW_* settings (tests switch them between passes): the current
// values of the rows flagged `plans`. No lock, no allocation.
uint64_t kw_knob_hash();

namespace knob_detail {  // what the readers below are made of (knobs.cpp); nothing else calls these

// The variable's current value (nullptr: unset), and a row's parsers over it. No lock, no allocation.
const char* env(const KnobRow& r);
bool parse_bool(const KnobRow& r);
int parse_int(const KnobRow& r);
double parse_double(const KnobRow& r);

// A latched row's value: parsed at its first read through either reader, one value per knob.
template <Knob K>
bool latched_bool() {
  static const bool v = parse_bool(kKnobs[K]);
  return v;
}
template <Knob K>
int latched_int() {
  static const int v = parse_int(kKnobs[K]);
  return v;
}

}  // namespace knob_detail

template <bool kPlanningOnly>
struct KnobReader {
  template <Knob K>
  static constexpr const KnobRow& row() {
    static_assert(!kPlanningOnly || kKnobs[K].plans, "planning reads only settings that are in the plan cache's key");
    return kKnobs[K];
  }
  template <Knob K>
  static bool on() {
    constexpr const KnobRow& r = row<K>();
    static_assert(r.kind == KnobKind::On || r.kind == KnobKind::Off || r.kind == KnobKind::Present);
    if constexpr (r.latched) return knob_detail::latched_bool<K>();
    else return knob_detail::parse_bool(r);
  }
  template <Knob K>
  static int num() {
    constexpr const KnobRow& r = row<K>();
    static_assert(r.kind == KnobKind::Int);
    if constexpr (r.latched) return knob_detail::latched_int<K>();
    else return knob_detail::parse_int(r);
  }
  template <Knob K>
  static double real() {
    constexpr const KnobRow& r = row<K>();
    static_assert(r.kind == KnobKind::Double && !r.latched);
    return knob_detail::parse_double(r);
  }
  template <Knob K>
  static bool is_set() {
    static_assert(!row<K>().latched);
    return knob_detail::env(row<K>()) != nullptr;
  }
  template <Knob K>
  static const char* str() {
    constexpr const KnobRow& r = row<K>();
    static_assert(r.kind == KnobKind::Str && !r.latched);
    const char* v = knob_detail::env(r);
    return v ? v : "";
  }
};

using PlanKnobs = KnobReader<true>;
#ifndef KW_PLANNING_TU
using Knobs = KnobReader<false>;
#endif

}  // namespace kw
