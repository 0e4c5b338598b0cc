// slots.hpp — bit-parallel evaluation of a policy list against one request.
//
// A validate pass answers a list of policy ids for every request of a batch
// (EvaluationEnvironment::validate, evaluation_environment.rs:546-594). The list compiles into
// chunks of up to 64 *slots* (one per plain policy or group member; equal settings share one) and
// the output columns that read them. A slot is one bit of a u64.
//
// Every string of a request is first classified into a small integer (kwdev.hpp classifiers). A
// chunk record then holds, per column class, the set of slots an entity of that class violates
// (tables below), so an entity's violation set is one table load — however many patterns the
// policies name. A slot's verdict is its *first* violation in object order (containers, then
// labels; the families' own order, DESIGN.md §2, oracle/kworacle.c fam_*), and the cost per request
// is O(entities + violations), not O(policies x entities).
//
// Shared by the device kernels (kernels.hip: entity-parallel in the tile kernel, the sequential
// walks below in the overflow kernel) and the host diagnostic kw_debug_host_walk (capi.cpp), which
// the CPU test suite uses to check the slot compiler against the oracle.
#pragma once
#include <cstdint>

#include "../../include/kwgpu.h"
#include "kwdev.hpp"

namespace kw {

constexpr uint32_t kSlots = 64;
constexpr uint32_t kArgWide = 0xffffu;  // ARG sentinel: the full value is in the pass's side data

// Per-class slot tables, each u64[nclass of its column] indexed by the column class.
enum SlotTab : uint32_t {
  T_NSOK = 0,  // COL_NS:  namespace slots whose valid_namespace is this class
  T_RA,        // COL_REG: trusted-repos slots whose registries.allow matches
  T_RR,        // COL_REG: ... registries.reject
  T_TR,        // COL_TAG: ... tags.reject
  T_IA,        // COL_IMG: ... images.allow
  T_IR,        // COL_IMG: ... images.reject
  T_NACAP,     // COL_CAP: strict psp-capabilities slots that allow neither the capability nor default-add it
  T_NAAA,      // COL_AA:  psp-apparmor slots that do not allow the profile
  T_DENY,      // COL_LK:  safe-labels slots that deny the key
  T_FAIL,      // COL_LV:  safe-labels slots whose constraint on the label's key the value fails
  NTAB
};

struct alignas(16) SlotHdr {
  uint64_t caps_strict;  // psp-capabilities slots without "*" in allowed_capabilities
  uint64_t caps;         // every psp-capabilities slot (mutation)
  uint64_t aa, lbl, ns, trs;
  uint64_t has_ra, has_ia;  // trusted-repos slots with a non-empty registries.allow / images.allow
  uint64_t priv[4];         // pod-privileged slots by (skip_init | skip_ephemeral << 1)
  uint64_t init;            // slots whose policy failed to initialise (group members: never ok)
  // local bits (per chunk): capabilities some slot requires dropped / adds by default ("ALL" always
  // has one when the chunk has psp-capabilities slots), and mandatory label keys
  uint64_t reqd_union, defa_union, all_bit, mand_union;
  uint64_t mand_one;  // slots whose mandatory list is a single key (its absence: index 0)
  uint32_t ncols, nslots, bytes, staged;  // bytes: whole record; staged: prefix the device keeps in LDS
  uint32_t tab_off[NTAB];                 // byte offset of each class table (0 = not emitted)
  uint32_t o_capmb, o_lkmb;               // u8 per COL_CAP / COL_LK class: its local bit, 0xff = none
  uint32_t o_reqd, o_defa, o_mand;        // u64[64] per local bit: the slots that list it
  uint32_t o_mlist;                       // u32 per slot: offset of its mandatory list (local bits in
                                          // settings order, 0xff-terminated), 0 = none
  uint32_t o_csoa;   // column arrays (kind | slot << 8, okw, mutw, rejb), each ncols rounded up to 4 u32
  uint32_t o_cols;   // ColInfo[ncols] (global memory on the device)
  uint32_t o_prog;   // group programs (global memory on the device)
  uint32_t nwide;    // group columns of this chunk with more than 15 members
  uint32_t o_mpack;  // u64 per slot: its first 8 mandatory local bits packed (0xff pad), 0 = none
  uint32_t pad1;
};
static_assert(sizeof(SlotHdr) % 16 == 0, "SlotHdr layout");

enum ColKind : uint32_t { CK_CONST = 0, CK_PLAIN = 1, CK_GROUP = 2, CK_TABLE = 3, CK_WIDE = 4 };

// One output column (a selected policy). PLAIN: verdict of slot `slot`. GROUP: the jump program at
// record offset prog_off over the member slots [slot, slot + nmem). TABLE: the truth table (u32
// entries, expr.hpp kGt*) at record offset prog_off over member slots [slot, slot + nmem), nmem <= 16;
// errw: the word of an evaluation error. WIDE: a wide group's placeholder (okw = 0), written after
// the pass by the wide-group combine kernel (groups.hpp WideGroupPass). CONST: the word `okw` whatever
// the request (initialisation error, group expression that is not a bool). okw / mutw / rejb: the
// service-level verdict word of an accepted, an accepted-and-mutated and a rejected vanilla response
// (reason/arg bits clear in rejb). wide: index of a > 15-member group in the pass's dense cause
// array (its causes do not fit ARG), else ~0.
struct alignas(16) ColInfo {
  uint32_t kind, slot, nmem, prog_off, prog_len, okw, mutw, rejb, wide, policy, errw, pad;
};
static_assert(sizeof(ColInfo) == 48, "ColInfo layout");

KW_HD inline uint32_t kw_ctz64(uint64_t x) { return (uint32_t)__builtin_ctzll(x); }
KW_HD inline uint32_t sat16(uint32_t a) { return a < kArgWide ? a : kArgWide; }
KW_HD inline uint32_t vword(uint32_t reason, uint32_t arg) { return (reason << 8) | (sat16(arg) << 16); }
KW_HD inline uint64_t bit_of(uint32_t b) { return b < 64u ? 1ull << b : 0ull; }  // 0xff: none

// Verdict word from a family result: the vanilla response plus validation_response_with_constraints
// (service.rs:160-208) for the Validate origin, vanilla for Audit (service.rs:108-116).
KW_HD inline uint32_t finish_word(uint32_t mode, uint32_t a2m, int origin, uint32_t reason, uint32_t arg, bool mutated) {
  uint32_t v = vword(reason, arg);
  const bool allowed = reason == 0;
  if (allowed) v |= KW_V_ALLOWED;
  if (mutated) v |= KW_V_MUTATED;
  uint32_t fst = allowed ? KW_FST_NONE : KW_FST_VANILLA;
  bool fallowed = allowed;
  if (origin == KW_ORIGIN_VALIDATE) {
    if (mode == KW_MODE_MONITOR) {
      fallowed = true;
      fst = KW_FST_NONE;
    } else if (mutated && !a2m) {
      fallowed = false;
      fst = KW_FST_MUTATION_REFUSED;
    }
  }
  if (fallowed) v |= KW_F_ALLOWED;
  if (mutated && fst == KW_FST_NONE && (origin == KW_ORIGIN_AUDIT || mode == KW_MODE_PROTECT)) v |= KW_F_PATCH;
  v |= fst << KW_F_STATUS_SHIFT;
  return v;
}
constexpr uint32_t kInitErrorWord = ((uint32_t)KW_FST_INIT_ERROR << KW_F_STATUS_SHIFT) | ((uint32_t)KW_R_INIT_ERROR << 8);
constexpr uint32_t kBypassWord = KW_V_ALLOWED | KW_F_ALLOWED | KW_BYPASS;

// The record's sections, resolved once (device: LDS or global pointers; host: the record bytes).
struct SlotView {
  const SlotHdr* h;
  const uint8_t* base;
  KW_HD const uint64_t* tab(uint32_t k) const { return (const uint64_t*)(base + h->tab_off[k]); }
  KW_HD uint64_t row(uint32_t k, uint32_t cls) const { return tab(k)[cls]; }
  KW_HD uint32_t capmb(uint32_t cls) const { return base[h->o_capmb + cls]; }
  KW_HD uint32_t lkmb(uint32_t cls) const { return base[h->o_lkmb + cls]; }
  KW_HD const uint64_t* reqd() const { return (const uint64_t*)(base + h->o_reqd); }
  KW_HD const uint64_t* defa() const { return (const uint64_t*)(base + h->o_defa); }
  KW_HD const uint64_t* mand() const { return (const uint64_t*)(base + h->o_mand); }
  KW_HD const uint8_t* mlist(uint32_t s) const { return base + ((const uint32_t*)(base + h->o_mlist))[s]; }
  KW_HD uint64_t mpack(uint32_t s) const { return ((const uint64_t*)(base + h->o_mpack))[s]; }
};

// OR of table rows over the set bits of `bits` (per 32-bit half, two independent row loads a round).
KW_HD inline uint64_t tab_or(const uint64_t* t, uint64_t bits) {
  uint64_t r = 0;
  for (uint32_t h = 0; h < 2; ++h) {
    uint32_t m = (uint32_t)(bits >> (32u * h));
    const uint64_t* th = t + 32u * h;
    while (m) {
      const uint32_t i = (uint32_t)__builtin_ctz(m);
      m &= m - 1u;
      const uint32_t j = m ? (uint32_t)__builtin_ctz(m) : i;
      m &= m - 1u;
      r |= th[i] | th[j];
    }
  }
  return r;
}

// Image classes of one container: the COL_REG entries (literal class, then one per DFA of the
// chain), the COL_TAG entries, the COL_IMG entries, in that order.
struct ImgLayout {
  uint32_t nreg, ntag, nimg;
  KW_HD uint32_t n() const { return nreg + ntag + nimg; }
};

// Trusted-repos reasons of one container (precedence order: registry not allowed, registry
// rejected, tag rejected, image not allowed, image rejected; oracle fam_trusted). `ic(j)`: the
// container's j-th image class.
template <class F>
KW_HD inline void trs_whys(const SlotView& sv, const ImgLayout& L, F ic, uint64_t why[5]) {
  uint64_t ra = 0, rr = 0, tr = 0, ia = 0, ir = 0;
  for (uint32_t j = 0; j < L.nreg; ++j) {
    const uint32_t c = ic(j);
    ra |= sv.row(T_RA, c);
    rr |= sv.row(T_RR, c);
  }
  for (uint32_t j = L.nreg; j < L.nreg + L.ntag; ++j) tr |= sv.row(T_TR, ic(j));
  for (uint32_t j = L.nreg + L.ntag; j < L.n(); ++j) {
    const uint32_t c = ic(j);
    ia |= sv.row(T_IA, c);
    ir |= sv.row(T_IR, c);
  }
  why[0] = sv.h->has_ra & ~ra;
  why[1] = rr;
  why[2] = tr;
  why[3] = sv.h->has_ia & ~ia;
  why[4] = ir;
}

// Privileged slots a container flagged `fl` violates.
KW_HD inline uint64_t priv_viol(const SlotHdr& h, uint32_t fl) {
  if (!(fl & KW_CTR_PRIVILEGED)) return 0ull;
  uint64_t v = h.priv[0];
  if (!(fl & KW_CTR_INIT)) v |= h.priv[1];
  if (!(fl & KW_CTR_EPHEMERAL)) v |= h.priv[2];
  if (!(fl & (KW_CTR_INIT | KW_CTR_EPHEMERAL))) v |= h.priv[3];
  return v;
}

// Mutated psp-capabilities slots of a container from its added / dropped local bits: a required
// drop missing (unless ALL is dropped) or a default add neither added nor dropped.
KW_HD inline uint64_t caps_mutation(const SlotView& sv, uint64_t addm, uint64_t dropm) {
  const SlotHdr& h = *sv.h;
  uint64_t mut = 0;
  if (!(dropm & h.all_bit)) mut |= tab_or(sv.reqd(), h.reqd_union & ~dropm);
  mut |= tab_or(sv.defa(), h.defa_union & ~(addm | dropm));
  return mut & h.caps;
}

// Index (settings order) of slot s's first mandatory key absent from `present` (local bits).
KW_HD inline uint32_t first_missing(const SlotView& sv, uint32_t s, uint64_t present) {
  const uint8_t* m = sv.mlist(s);
  uint32_t i = 0;
  for (;; ++i) {
    const uint32_t b = m[i];
    if (b == 0xffu || !((present >> b) & 1ull)) break;
  }
  return i;
}

// first_missing from the slot's packed list (one u64 load for lists of up to 8 keys; longer lists
// continue in mlist): the same index.
KW_HD inline uint32_t first_missing_packed(const SlotView& sv, uint32_t s, uint64_t packed, uint64_t present) {
  for (uint32_t i = 0; i < 8; ++i) {
    const uint32_t b = (uint32_t)(packed >> (8u * i)) & 0xffu;
    if (b == 0xffu || !((present >> b) & 1ull)) return i;
  }
  const uint8_t* m = sv.mlist(s);
  uint32_t i = 8;
  while (m[i] != 0xffu && ((present >> m[i]) & 1ull)) ++i;
  return i;
}

// Violation sink of the sequential walks: the word (16-bit ARG, saturated) and the full argument.
struct ViolSink {
  uint32_t* vw;
  uint32_t* va;  // may be null
  // (the mask is walked as two 32-bit halves: one find-first-set and one clear per slot)
  KW_HD void put(uint64_t nw, uint32_t reason, uint32_t arg) const {
    const uint32_t w = vword(reason, arg);
#ifdef KW_PUT64
    while (nw) {
      const uint32_t s = kw_ctz64(nw);
      vw[s] = w;
      if (va) va[s] = arg;
      nw &= nw - 1;
    }
    return;
#endif
#ifndef KW_PUT2  // two slots a loop trip (the second repeats the first when the half runs out: idempotent)
#define KW_PUT2 1
#endif
    for (uint32_t h = 0; h < 2; ++h) {
      uint32_t m = (uint32_t)(nw >> (32u * h));
      while (m) {
        const uint32_t s = 32u * h + (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        uint32_t s2 = s;
        if (KW_PUT2 && m) {
          s2 = 32u * h + (uint32_t)__builtin_ctz(m);
          m &= m - 1u;
        }
        vw[s] = w;
        vw[s2] = w;
        if (va) {
          va[s] = arg;
          va[s2] = arg;
        }
      }
    }
  }
};

// ---- sequential walks over one request (host diagnostic and the overflow kernel). The accessor
// S gives the request's structure (rf / coff / loff / cflags / cadd / cdrop) and the classes of its
// strings (ns / aa / capadd / capdrop / lk / lv(l, j) / img(c, j)) with img layout `il` and nlv()
// classes per label value. Each walk returns the rejected slots of its families.

// walk A: pod-privileged + psp-capabilities (validation, then mutation), containers in order.
// *mut_out gets the mutated-and-not-rejected psp-capabilities slots.
template <class S>
KW_HD uint64_t walk_privileged_caps(const S& src, const SlotView& sv, uint64_t r, const ViolSink& vs, uint64_t* mut_out) {
  const SlotHdr& h = *sv.h;
  uint64_t rej = 0, mut = 0;
  const uint64_t privany = h.priv[0] | h.priv[1] | h.priv[2] | h.priv[3];
  if ((src.rf(r) & KW_REQ_HAS_PODSPEC) && (privany | h.caps)) {
    const uint32_t cb = src.coff(r), ce = src.coff(r + 1);
    const uint32_t kfirst = src.cadd(cb);
    for (uint32_t c = cb; c < ce; ++c) {
      const uint32_t fl = src.cflags(c);
      const uint64_t pv = priv_viol(h, fl) & ~rej;
      vs.put(pv, KW_R_PRIVILEGED, c - cb);
      rej |= pv;
      if (h.caps) {
        const uint32_t k0 = src.cadd(c), k1 = src.cadd(c + 1);
        uint64_t addm = 0, dropm = 0;
        for (uint32_t k = k0; k < k1; ++k) {
          const uint32_t cls = src.capadd(k);
          addm |= bit_of(sv.capmb(cls));
          const uint64_t nw = (h.caps_strict ? sv.row(T_NACAP, cls) : 0ull) & ~rej;
          vs.put(nw, KW_R_CAP_NOT_ALLOWED, k - kfirst);  // index in the request's add lists, flattened
          rej |= nw;
        }
        for (uint32_t k = src.cdrop(c), k1d = src.cdrop(c + 1); k < k1d; ++k) dropm |= bit_of(sv.capmb(src.capdrop(k)));
        mut |= caps_mutation(sv, addm, dropm);
      }
    }
  }
  *mut_out = mut & ~rej;
  return rej;
}

// walk B: psp-apparmor + trusted-repos, containers in order.
template <class S>
KW_HD uint64_t walk_apparmor_images(const S& src, const SlotView& sv, uint64_t r, const ViolSink& vs) {
  const SlotHdr& h = *sv.h;
  uint64_t rej = 0;
  if ((src.rf(r) & KW_REQ_HAS_PODSPEC) && (h.aa | h.trs)) {
    const uint32_t cb = src.coff(r), ce = src.coff(r + 1);
    for (uint32_t c = cb; c < ce; ++c) {
      const uint32_t ci = c - cb;
      const uint32_t fl = src.cflags(c);
      if (h.aa && (fl & KW_CTR_HAS_APPARMOR)) {
        const uint64_t nw = sv.row(T_NAAA, src.aa(c)) & ~rej;
        vs.put(nw, KW_R_APPARMOR, ci);
        rej |= nw;
      }
      if (h.trs && (fl & KW_CTR_HAS_IMAGE)) {
        uint64_t why[5];
        trs_whys(sv, src.il, [&](uint32_t j) { return src.img(c, j); }, why);
        for (uint32_t k = 0; k < 5; ++k) {
          const uint64_t nw = why[k] & h.trs & ~rej;
          vs.put(nw, KW_R_REG_NOT_ALLOWED + k, ci);
          rej |= nw;
        }
      }
    }
  }
  return rej;
}

// V_l of one label: the safe-labels slots that deny its key or whose constraint on it the value fails.
template <class S>
KW_HD uint64_t label_viol(const S& src, const SlotView& sv, uint32_t l) {
  const uint32_t k = src.lk(l);
  if (!k) return 0ull;
  uint64_t v = sv.row(T_DENY, k);
  for (uint32_t j = 0; j < src.nlv(); ++j) {
    const uint32_t c = src.lv(l, j);
    if (c != 0xffffu) v |= sv.row(T_FAIL, c);
  }
  return v;
}

// walk C: safe-labels (denied, then constrained, label by label in object order; then the first
// missing mandatory key, settings order).
template <class S>
KW_HD uint64_t walk_labels(const S& src, const SlotView& sv, uint64_t r, const ViolSink& vs) {
  const SlotHdr& h = *sv.h;
  if (!h.lbl) return 0;
  uint64_t rej = 0, present = 0;
  const uint32_t lb = src.loff(r), le = src.loff(r + 1);
  for (uint32_t l = lb; l < le; ++l) {
    const uint32_t k = src.lk(l);
    if (!k) continue;
    present |= bit_of(sv.lkmb(k));
    const uint64_t den = sv.row(T_DENY, k);
    const uint64_t nv = label_viol(src, sv, l) & ~rej;
    vs.put(nv & den, KW_R_LABEL_DENIED, l - lb);
    vs.put(nv & ~den, KW_R_LABEL_CONSTRAINT, l - lb);
    rej |= nv;
  }
  uint64_t nw = tab_or(sv.mand(), h.mand_union & ~present) & ~rej;
  rej |= nw;
  while (nw) {
    const uint32_t s = kw_ctz64(nw);
    nw &= nw - 1;
    vs.put(1ull << s, KW_R_LABEL_MANDATORY, first_missing(sv, s, present));
  }
  return rej;
}

// walk D: namespace allow-list.
template <class S>
KW_HD uint64_t walk_namespace(const S& src, const SlotView& sv, uint64_t r, const ViolSink& vs) {
  const SlotHdr& h = *sv.h;
  if (!h.ns) return 0;
  const uint64_t ok = (src.rf(r) & KW_REQ_HAS_NAMESPACE) ? sv.row(T_NSOK, src.ns(r)) : 0ull;
  const uint64_t nw = h.ns & ~ok;
  vs.put(nw, KW_R_NAMESPACE, 0);
  return nw;
}

// namespace bypass (service.rs:40-71): an AdmissionRequest in the always-accept namespace
KW_HD inline bool is_bypass(uint32_t rf, uint32_t ns_cls, uint32_t bypass_cls) {
  return bypass_cls != 0 && !(rf & KW_REQ_RAW) && (rf & KW_REQ_HAS_NAMESPACE) && ns_cls == bypass_cls;
}

// Group jump program (kwdev.hpp GOp) over the member results `ok` (bit s: member s accepted and did
// not mutate). Returns the expression's value; *causes = the members rhai would have called that
// rejected (evaluation_environment.rs:979-1042). (The wide path's programs: groupvm.hpp.)
KW_HD inline bool run_group_prog(const uint8_t* prog, uint32_t len, uint64_t ok, uint64_t* causes) {
  uint64_t vals = 0, cz = 0;
  uint32_t sp = 0;
  for (uint32_t pc = 0; pc < len;) {
    const uint32_t op = prog[pc++];
    if (op == G_CONST0 || op == G_CONST1 || op == G_CALL) {
      uint64_t v = op == G_CONST1 ? 1ull : 0ull;
      if (op == G_CALL) {
        const uint32_t s = prog[pc++];
        v = (ok >> s) & 1ull;
        if (!v) cz |= 1ull << s;
      }
      vals = (vals & ~(1ull << sp)) | (v << sp);
      ++sp;
    } else if (op == G_NOT) {
      vals ^= 1ull << (sp - 1);
    } else if (op == G_JT || op == G_JF) {
      const uint32_t t = (uint32_t)prog[pc] | ((uint32_t)prog[pc + 1] << 8);
      pc += 2;
      const bool top = (vals >> (sp - 1)) & 1ull;
      if (top == (op == G_JT)) pc = t;
      else --sp;
    } else {  // G_EQ / G_NE
      --sp;
      const uint64_t b = (vals >> sp) & 1ull, a = (vals >> (sp - 1)) & 1ull;
      const uint64_t v = op == G_EQ ? (uint64_t)(a == b) : (uint64_t)(a != b);
      vals = (vals & ~(1ull << (sp - 1))) | (v << (sp - 1));
    }
  }
  *causes = cz;
  return vals & 1ull;
}

// Verdict word of one output column for one request. rej / mut: the request's rejected and mutated
// slots; vw: its violation words (valid where rej is set); prog: the record's programs (prog_off
// is record-relative); *wide gets the cause mask of a > 15-member group.
KW_HD inline uint32_t column_word(const ColInfo& ci, uint64_t rej, uint64_t mut, uint64_t init, const uint32_t* vw,
                                  const uint8_t* rec, uint64_t* wide) {
  if (ci.kind == CK_PLAIN) {
    if ((rej >> ci.slot) & 1ull) return ci.rejb | vw[ci.slot];
    return ((mut >> ci.slot) & 1ull) ? ci.mutw : ci.okw;
  }
  if (ci.kind == CK_GROUP) {
    const uint64_t mask = ci.nmem >= 64 ? ~0ull : (1ull << ci.nmem) - 1ull;
    const uint64_t ok = (~(rej | mut | init) >> ci.slot) & mask;
    uint64_t causes;
    if (run_group_prog(rec + ci.prog_off, ci.prog_len, ok, &causes)) return ci.okw;
    if (ci.nmem > 15) {  // 16 causes could read as the ARG sentinel
      *wide = causes;
      return ci.rejb | vword(KW_R_GROUP, kArgWide);
    }
    return ci.rejb | vword(KW_R_GROUP, (uint32_t)causes);
  }
  if (ci.kind == CK_TABLE) {
    const uint32_t ok = (uint32_t)((~(rej | mut | init) >> ci.slot) & ((1ull << ci.nmem) - 1ull));
    const uint32_t e = ((const uint32_t*)(rec + ci.prog_off))[ok];
    if (e & 2u) return ci.errw;  // kGtError
    if (e & 1u) return ci.okw;   // kGtValue
    const uint32_t causes = e >> 16;
    if (ci.nmem > 15) {
      *wide = causes;
      return ci.rejb | vword(KW_R_GROUP, kArgWide);
    }
    return ci.rejb | vword(KW_R_GROUP, causes);
  }
  return ci.okw;
}

}  // namespace kw
