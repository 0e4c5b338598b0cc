// kernels.hpp — launch interface of the device hot path (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kwdev.hpp"
#include "slots.hpp"

namespace kw {

// String columns a tile stages (each feeds the classification of one or more request columns).
enum Str : uint32_t { S_NS = 0, S_IMG, S_AA, S_CAPADD, S_CAPDROP, S_LK, S_LV, NSTR };

// Pass-side data of arguments that do not fit a verdict word's 16-bit ARG (kArgWide): an entity
// index >= 65535 (only requests beyond the tile capacities have one: the overflow kernel appends a
// record) and the cause mask of a > 15-member group (dense [row][nwide] array).
struct WideRec {
  uint32_t row_lo, row_hi, policy, value;
};

struct EvalArgs {
  const uint8_t* blob;
  uint64_t nrows;
  uint64_t ndesc;  // tile descriptors (TileDesc) to walk
  uint32_t npol;   // verdict words per row (all-pairs: the policy list; rows mode: 1)
  int32_t origin;
  const uint8_t* req_flags;
  const uint32_t* ctr_off;
  const uint32_t* lbl_off;
  const uint8_t* ctr_flags;
  const uint32_t* capadd_off;
  const uint32_t* capdrop_off;
  uint32_t* out;
  uint32_t* sched;  // per-XCD tile counters (256 u32 + 256 u32 done counts), nullptr = static schedule
  uint32_t sched_static;  // with sched: a slot's first S tiles are strided, the counters draw the rest (S >= 2)
  // overflow path: per-string classes in HBM (absolute entity indices), the wide-argument list
  uint16_t *g_ns, *g_aa, *g_img, *g_capadd, *g_capdrop, *g_lk, *g_lv;
  // NFA elements (kwdev.hpp DevNfa): their classes, computed by nfa_classify_kernel before the tile
  // kernel, [label][nlv] and [container][il.n()] at the element's chain position (nullptr = none)
  const uint16_t *nfa_lv, *nfa_img;
  uint32_t* wide_count;
  WideRec* wide_rec;
  uint32_t wide_cap;
  uint64_t* wide_groups;  // dense [row][nwide] cause masks
  uint32_t nwide;
  const uint32_t* rowcol;  // rows mode: per row (chunk << 16) | column, all-pairs: nullptr
  // diagnostics (KW_TILE_DEBUG & 512): per workgroup kPhaseWords u64: shader-clock cycles of thread
  // 0 summed over its tiles [staging P0, classify P1, derive D, walk P2, verdicts P3 + next tile,
  // tiles, whole workgroup, table staging], then the kSegWords segment clocks (Seg) summed over the
  // workgroup's waves; nullptr = off
  uint64_t* phase;
};
// Per-wave segment clocks of the timing instantiation: P1 / P2 item segments (wave-uniform per
// loop iteration), each phase's busy time and its barrier wait.
enum Seg : uint32_t {
  SG_P1_LABEL = 0, SG_P1_CAPSTR, SG_P1_CTR, SG_P1_IMAGE, SG_P1_REQ, SG_P2_CTR, SG_P2_LABEL, SG_P2_REQ,
  SG_P1_BUSY, SG_P1_WAIT, SG_P2_BUSY, SG_P2_WAIT, SG_P0_WAIT, SG_P3_BUSY, SG_P3_WAIT,
  SG_START,  // the workgroup's start (s_memrealtime, 100 MHz): residency of the grid
  // P0 issue: tile loop top to the descriptor's `fits`; the jobs' spans (copy_span on every lane); the
  // wave's job loop (readlanes and copies)
  SG_P0_TOP, SG_P0_REQ, SG_P0_STR,
  SG_END,  // the workgroup's end after its last tile (s_memrealtime): how evenly an XCD's slots finish
  kSegWords = 20
};
// A workgroup's words fill whole 128-byte lines: neighbouring workgroups run on different XCDs, and
// so no two L2s hold the same line of counters.
constexpr uint32_t kPhaseWords = 32;
static_assert(kPhaseWords >= 8 + kSegWords && kPhaseWords % 16 == 0, "phase words per workgroup: whole lines");

// Slot kernel geometry: one tile = up to 64 requests (one lane per request where a lane walks a
// request), 256 threads.
constexpr uint32_t kSlotRows = 64;
#ifndef KW_THREADS  // threads per tile workgroup (build-time A/B)
#define KW_THREADS 256
#endif
constexpr uint32_t kSlotThreads = KW_THREADS;
// Workgroups of `bytes` dynamic LDS one gfx950 CU holds at once (256 threads, LDS-bound): the CU's
// 160 KiB are allocated in 1280-byte granules, 128 of them — measured (scripts/lds_occ.hip,
// profiles/r05_lds_residency.txt): 53760 B holds 3, 53768 B holds 2, 32000 B 5, 32004 B 4. The HIP
// occupancy API's floor(160 KiB / bytes) overstates it between granule boundaries (r05: a C5 heavy
// layout of 53664 B planned at 3 ran at 2, a third of its grid waiting for the first two-thirds).
constexpr uint32_t kLdsGranule = 1280, kLdsGranules = 128;
constexpr uint32_t lds_workgroups_per_cu(uint32_t bytes) {
  const uint32_t g = (bytes + kLdsGranule - 1) / kLdsGranule;
  return g ? kLdsGranules / g : kLdsGranules;
}
// Families a tile-kernel instantiation carries (TileArgs::feat).
constexpr uint32_t kFeatImg = 1, kFeatLbl = 2, kFeatCtr = 4, kFeatGrp = 8, kFeatAll = 15;
// A pass whose classifiers hold NFA elements runs the one instantiation that reads their classes
// (kFeatAll | kFeatNfa): no other instantiation carries that code.
constexpr uint32_t kFeatNfa = 16;
// Tiles with many containers per request (TileArgs::ctr_ranges) in the label / container family set
// with LDS tables (C5's heavy region): P2 takes a container's predecessor sets from a segmented
// wave OR-scan. Its own instantiation, so the others (C4's) keep their code and registers.
constexpr uint32_t kFeatRng = 32;
#ifndef KW_PREFETCH  // tile kernel: the code of the next-tile L2 prefetch (run only when the plan asks:
#define KW_PREFETCH 1   // plan.cpp l2_prefetch, off by default; r02 s60: running it cost C4 0.3442 vs 0.3294 ms)
#endif
#ifndef KW_PF_LANES  // lanes per wave issuing the next tile's L2 prefetch (its LDS landing line: 4 B each)
#define KW_PF_LANES 64
#endif
constexpr uint32_t kPfLanes = KW_PF_LANES;
constexpr uint32_t kMaxChunks = 8;  // chunks of one launch (<= 512 slots); longer lists take several launches

struct ChunkArgs {
  const uint8_t* rec;  // device copy of the SlotHdr record (ColInfo and programs are read here)
  uint32_t o_lds;      // LDS offset of the record's staged prefix (tables in LDS), else 0
  uint32_t col0, ncols, vec4;
  uint64_t init;
};

// One array a tile stages (P0 of the tile kernel): the column's device address, where it lands in
// LDS, and how the tile's span of it follows from two words of the tile's descriptor (TileDesc as
// u32 words). The planner fills one table per launch (plan.cpp build_copy_jobs); in the kernel lane j
// holds job j (three registers), so every job's span is one round of the same arithmetic
// (copy_span) on all lanes.
// code: bits 0-4 / 5-9 the descriptor words B and E; kCjRel: E counts from B (else E is the end);
// kCjReq: B is a request index, its high half in TileDesc::r0hi; kCjQuad: the span is counted in
// pieces of 4 elements, rounded up (byte arrays copied as dwords); kCjAlign: B is first aligned down
// to a piece; kCjPlus1: one piece more (an offsets array has n + 1 entries); kCjElem4: 4-byte
// elements, else bytes; kCjX4: 16-byte pieces, else dwords; bits 18-31: the LDS destination / 16.
struct CopyJob {
  uint64_t base;
  uint32_t code;
  uint32_t pad;
};
constexpr uint32_t kCjRel = 1u << 10, kCjReq = 1u << 11, kCjQuad = 1u << 12, kCjAlign = 1u << 13, kCjPlus1 = 1u << 14,
                   kCjElem4 = 1u << 15, kCjX4 = 1u << 16, kCjLdsShift = 18;
constexpr uint32_t copy_code(uint32_t wb, uint32_t we, uint32_t lds, uint32_t flags) {
  return wb | (we << 5) | flags | ((lds >> 4) << kCjLdsShift);
}
KW_HD constexpr uint32_t copy_lds(uint32_t code) { return (code >> kCjLdsShift) << 4; }
struct CopySpan {
  uint64_t byte_off;  // from CopyJob::base
  uint32_t count;     // pieces (dwords, or 16-byte vectors with kCjX4)
};
// The span of a job in a tile: b = desc[code & 31], e = desc[(code >> 5) & 31], r0hi = TileDesc::r0hi.
// Selections are masks and shifts, not branches: the lanes of a wave hold jobs of every kind.
KW_HD inline CopySpan copy_span(uint32_t code, uint32_t b, uint32_t e, uint32_t r0hi) {
  const uint32_t sh = (code >> 11) & 2u, bsh = (code >> 14) & 2u, rnd = (1u << sh) - 1u;  // kCjQuad, kCjElem4: 0 or 2
  const uint32_t rel = 0u - ((code >> 10) & 1u), req = 0u - ((code >> 11) & 1u), al = 0u - ((code >> 13) & 1u);
  const uint32_t b0 = b & ~(rnd & al);
  const uint32_t end = e + (b & rel);
  CopySpan s;
  s.count = ((end - b0 + rnd) >> sh) + ((code >> 14) & 1u);
  s.byte_off = (((uint64_t)(r0hi & req) << 32) | b0) << bsh;
  return s;
}
constexpr uint32_t kMaxCopyJobs = 6 + 2 * NSTR;

// Per-launch geometry and LDS layout. Lives in device memory; the kernel reads it with scalar loads.
struct TileArgs {
  uint32_t rows;                  // requests per tile
  uint32_t cmax, kmax, lmax;      // container / capability / label capacity of a staged tile
  uint32_t o_rf, o_coff, o_loff, o_cflags, o_cadd, o_cdrop;  // staged headers (LDS byte offsets)
  // per-entity classes (u16): namespace [rows], AppArmor [cmax], image [cmax][il.n()], added /
  // dropped capabilities [kmax], label keys [lmax], label values [lmax][nlv]. In a single-chunk
  // pass whose value classes fold into the walk, o_lv's region doubles as the label-pair helper
  // lanes' per-wave 128-B mailboxes (kernels.hip label_pairs: needs lmax * nlv * 2 >= 4 x 128)
  uint32_t o_ns, o_aa, o_img, o_capadd, o_capdrop, o_lk, o_lv;
  ImgLayout il;
  uint32_t nlv;
  uint32_t need;  // bit per Str: the pass classifies that string column
  uint32_t o_vadd, o_vl, o_vc, o_vtr;  // u64 violation sets: per added capability, per label, per container (2)
  uint32_t o_own_c, o_own_l;           // u8 tile-local request of each staged container / label
  uint32_t o_rej, o_mut, o_byp;        // per-request results: rejected / mutated slots, bypass flag
  uint32_t o_nx;                       // u32[4]: the tile after next (dynamic schedule), double-buffered; P1 / P2 block counters
  uint32_t o_desc;                     // TileDesc[2]: this tile's and the next tile's descriptor
  uint32_t o_pf;                       // 4 x kPfLanes B: LDS-DMA landing of the L2 prefetch (never read)
  uint32_t prefetch;                   // warm L2 with the next tile (small tiles at >= 3 workgroups per CU)
  uint32_t feat;                       // kFeat* families of the launch (selects the kernel instantiation)
  uint32_t ctr_ranges;                 // many containers per request: P2 ORs predecessor ranges four a round
  uint32_t o_sa;                       // u32[NSTR]: the tile's staged byte start per string column
  uint32_t o_vw, vw_stride;            // violation words [rows][vw_stride] (aliases the staged strings)
  uint32_t o_so[NSTR], o_sb[NSTR], sb_cap[NSTR];  // staged string offsets / bytes (0 = not staged)
  const uint32_t* s_off[NSTR];
  const uint8_t* s_bytes[NSTR];
  // P0's copy jobs: the six request / container arrays, then offsets and bytes of each staged string
  // column, ordered so that job j on wave j % 4 balances the waves' copy instructions
  CopyJob jobs[kMaxCopyJobs];
  uint32_t njobs;
  // column classifiers: LDS offsets when staged (lds_tables), blob offsets always
  uint32_t lds_tables;
  uint32_t lit_lds[NCOL], dfa_lds[NCOL], kv_lds;
  uint32_t lit_blob[NCOL], dfa_blob[NCOL], kv_blob, nlk;
  uint32_t nstage;
  uint32_t stage_blob[NCOL + kMaxChunks], stage_lds[NCOL + kMaxChunks], stage_bytes[NCOL + kMaxChunks];
  uint32_t bypass_cls, docker_io_cls, latest_cls;
  uint32_t nchunk;
  ChunkArgs chunk[kMaxChunks];
  uint32_t rows_mode;
  uint32_t debug;  // diagnostics: bit0 skip classification, bit1 skip walk, bit2 skip output; 512 phase
                  // clocks; 1024 skip mandatory labels, 2048 skip label-value DFAs, 4096 skip predecessor ORs,
                  // 8192 skip capability mutations (P2), 16384 skip container / label violation words (P2),
                  // 32768 / 65536 skip the image DFA chains / literal lookups (P1)
  uint32_t lds_bytes;
  uint32_t generic;  // KW_TILE_GENERIC: the launch takes the generic kernel whatever its shape (host side only)
};

// The production shape of a launch: the ordinary all-pairs pass of a label / container policy set,
// whose tile kernel is compiled with these values as constants (evaluate_tiles_kernel's PROD, the
// shape_* accessors in kernels.hip): no ablation bit, one chunk, all pairs, no L2 prefetch, 16-byte
// verdict stores with a power-of-two number of column groups that divides the workgroup, tables in
// LDS, no NFA element, and the family set one of the two that have such a kernel (with kFeatRng
// exactly where the tiles take predecessor ranges). timing: the pass runs the phase clocks
// (EvalArgs::phase), which stay on the generic kernel. The launch (tile_kernel_kind) and the tests
// (kw_debug_prod_shape) decide by this one function.
inline bool tile_prod_shape(const TileArgs& t, bool timing) {
  const uint32_t feat = t.feat & (kFeatAll | kFeatNfa | kFeatRng);
  if (feat != (kFeatLbl | kFeatCtr) && feat != (kFeatLbl | kFeatCtr | kFeatRng)) return false;
  if ((t.ctr_ranges != 0) != ((feat & kFeatRng) != 0)) return false;
  if (timing || t.generic || t.debug != 0 || !t.lds_tables) return false;
  if (t.nchunk != 1 || t.rows_mode || t.prefetch) return false;
  const ChunkArgs& c = t.chunk[0];
  const uint32_t G = c.ncols / 4u;
  return c.vec4 && c.ncols % 4u == 0 && G >= 1 && (G & (G - 1u)) == 0 && G <= kSlotThreads;
}

// Per-tile geometry, precomputed on the host from the batch's offsets (one s_load burst per tile
// instead of a chain of dependent global loads): entity ranges, the 16-B aligned byte range of each
// staged string column, and whether the tile fits the LDS capacities.
// A tile is a run of at most kSlotRows requests; runs that exceed the LDS capacities are halved
// until they fit, and single requests that still do not fit go to the overflow kernels.
struct alignas(16) TileDesc {
  uint32_t cb, ce, lb, le, kab, kae, kdb, kde;
  uint32_t sa[NSTR];  // staged column: first byte (16-B aligned) of the tile's strings in the pool
  uint32_t pad0;
  uint32_t nv[NSTR];  //                16-B vectors to copy
  uint32_t fits;
  uint32_t r0lo, r0hi, nr;  // first request (64-bit) and request count
  uint32_t pad[4];
};
static_assert(sizeof(TileDesc) == 128, "TileDesc layout");

// The tile schedule's index arithmetic, one statement of it for the kernel and for the host, which
// counts a launch's tiles per slot by it (pass.cpp build_descs): workgroup b of a grid runs on XCD b % nx and is that XCD's slot
// b / nx; the XCD serves the contiguous descriptors [t_lo, t_hi) of the launch's ndesc, and on the
// strided schedule slot j's k-th tile is the descriptor at t_lo + j + k * wpx.
struct TileSlot {
  uint32_t nx, xcd, slot, wpx;  // XCDs in use; the workgroup's XCD and slot in it; the XCD's workgroups
  uint64_t t_lo, t_hi;
};
KW_HD inline TileSlot tile_slot(uint64_t ndesc, uint32_t grid, uint32_t b) {
  TileSlot s;
  s.nx = grid < 8u ? grid : 8u;
  s.xcd = b % s.nx;
  s.slot = b / s.nx;
  s.wpx = (grid - s.xcd + s.nx - 1u) / s.nx;  // workgroups b < grid with b % nx == xcd
  s.t_lo = ndesc * s.xcd / s.nx;
  s.t_hi = ndesc * (s.xcd + 1u) / s.nx;
  return s;
}
// The descriptor a slot runs as its k-th tile on the strided schedule (a tile only while < t_hi).
KW_HD inline uint64_t tile_at(const TileSlot& s, uint32_t k) { return s.t_lo + s.slot + (uint64_t)k * s.wpx; }
// The counter schedule with S static rounds (EvalArgs::sched_static): a slot's tiles k < S are its
// strided ones, and the XCD's counter hands out the tail [tail_lo, t_hi) one descriptor at a time to
// whichever slot asks next. Every descriptor of [t_lo, t_hi) is either one slot's static tile
// (below tail_lo: slot (i - t_lo) % wpx, tile (i - t_lo) / wpx) or in the tail, never both. With
// S above the XCD's whole rounds the tail is empty and a slot's last static tiles do not exist. (The
// kernel fixes a slot's first two tiles before its first fetch, so it takes S >= 2 only; the
// arithmetic holds for any S.)
KW_HD inline uint64_t tile_tail_lo(const TileSlot& s, uint32_t S) {
  const uint64_t lo = s.t_lo + (uint64_t)S * s.wpx;
  return lo < s.t_hi ? lo : s.t_hi;
}
// Whole rounds of a launch: the least over its XCDs of the rounds in which every slot has a tile.
// S <= tile_whole_rounds means every static tile exists.
KW_HD inline uint64_t tile_whole_rounds(uint64_t ndesc, uint32_t grid) {
  uint64_t q = ~0ull;
  const uint32_t nx = grid < 8u ? grid : 8u;
  for (uint32_t x = 0; x < nx; ++x) {
    const TileSlot s = tile_slot(ndesc, grid, x);
    const uint64_t r = (s.t_hi - s.t_lo) / s.wpx;
    q = r < q ? r : q;
  }
  return nx ? q : 0;
}

// Estimated cost of a tile in wave-cycles, from its item counts: P1 and P2 run their items in
// 64-lane blocks, one wave a block, and a block costs its longest chain however few lanes it fills
// (DESIGN.md §5), so a segment costs per block, not per item. The planner cuts tiles where the cost
// per request is least (pass.cpp build_descs).
struct TileCostW {
  uint32_t fixed, req, lbl, ctr, cap;  // per tile; per block of requests / labels / containers / capability strings
};
KW_HD constexpr uint32_t tile_blocks(uint32_t items) { return (items + 63u) / 64u; }
KW_HD constexpr uint64_t tile_cost(const TileCostW& w, uint32_t nreq, uint32_t nlbl, uint32_t nctr, uint32_t ncap) {
  return (uint64_t)w.fixed + (uint64_t)w.req * tile_blocks(nreq) + (uint64_t)w.lbl * tile_blocks(nlbl) +
         (uint64_t)w.ctr * tile_blocks(nctr) + (uint64_t)w.cap * tile_blocks(ncap);
}
// The weights of a launch's family set (TileArgs::feat) and classified string columns (need).
// Label / container families (C4's instantiation), from the committed segment clocks of
// profiles/r07_p0_segments.txt ("change" rows: cycles per wave and tile, x 4 waves, over the mean
// blocks per tile of that batch — 4.07 label, 2.47 container, 3.47 capability-string, 1 request):
//   label    (P1 label 7435 + P2 label 2702) x 4 / 4.07 =  9.96 k
//   ctr      (P1 ctr   1758 + P2 ctr   4790) x 4 / 2.47 = 10.6 k
//   cap       P1 capstr 2382                 x 4 / 3.47 =  2.75 k
//   request  (P1 req    646 + P2 req   1467) x 4        =  8.45 k
//   fixed     tile 32950 x 4 less the four segments above = 47.0 k
// The r08 refit on two other boxes (profiles/r08_tile_cost_fit.txt) gave each within 0.3 % and
// within 6 % (that box's clocks run 2.7 % higher throughout); the weights stay.
// Image family: a container also costs its image chain in P1; profiles/r03_segment_clocks.txt, C2:
// (P1 image 18020 + P2 ctr 3960) x 4 / 2.47 = 35.6 k per container block.
KW_HD constexpr TileCostW tile_cost_weights(uint32_t feat, uint32_t need) {
  TileCostW w{47000u, 8450u, 0u, 0u, 0u};
  if ((feat & kFeatLbl) && (need & (1u << S_LK))) w.lbl = 9960u;
  if (feat & kFeatCtr) w.ctr = 10600u;
  if ((feat & kFeatCtr) && (need & (1u << S_CAPADD))) w.cap = 2750u;
  if ((feat & kFeatImg) && (need & (1u << S_IMG))) w.ctr = 35600u;
  return w;
}

// Fills T->jobs / njobs (plan.cpp) from T's LDS layout and string columns and the batch's six
// request / container arrays cols[] = {req_flags, ctr_off, lbl_off, ctr_flags, capadd_off, capdrop_off}.
void build_copy_jobs(TileArgs* T, const void* const cols[6]);

// The grid a launch of the tile kernel really runs: the planner's, clamped to the workgroups the
// device holds at once of the launch's instantiation (timing: the diagnostics one, whose registers
// allow fewer) and LDS size. The kernel's schedule arithmetic is in terms of this grid (gridDim.x),
// so what the host derives for a launch (sched_static_rounds, the phase report) takes it from here.
// Needs the launch's device current; with no device the grid comes back as it is.
// print: with KW_TILE_DEBUG & 256, the [kw tile] line of the launch.
uint32_t tile_launch_grid(const TileArgs& t, bool timing, uint32_t grid, bool print = false);
// The kernel a launch of `t` takes: the production-shape instantiation where tile_prod_shape holds,
// else the generic one of its family set. launch_evaluate_tiles and tile_launch_grid choose by it,
// and a pass reports it per launch (kw_debug_last_kernels).
constexpr uint32_t kTileKernelGeneric = 0, kTileKernelProd = 1;
uint32_t tile_kernel_kind(const TileArgs& t, bool timing);

// The variant of a launch: the four arguments the dispatch (kernels.hip tile_fn) is called with, as
// one word (kw_debug_last_variants, kw_debug_plan_variants): bits 0-5 the family and flag bits
// feat & (kFeatAll | kFeatNfa | kFeatRng), then LDS tables, phase clocks, production shape.
struct TileVariant {
  bool ldst, timing;
  uint32_t feat;
  bool prod;
};
constexpr uint32_t kVarFeatMask = kFeatAll | kFeatNfa | kFeatRng, kVarLdst = 1u << 8, kVarTiming = 1u << 9, kVarProd = 1u << 10;
constexpr uint32_t tile_variant_word(const TileVariant& v) {
  return (v.feat & kVarFeatMask) | (v.ldst ? kVarLdst : 0u) | (v.timing ? kVarTiming : 0u) | (v.prod ? kVarProd : 0u);
}
constexpr TileVariant tile_variant_of(uint32_t w) {
  return TileVariant{(w & kVarLdst) != 0, (w & kVarTiming) != 0, w & kVarFeatMask, (w & kVarProd) != 0};
}
inline uint32_t tile_feat(const TileArgs& t) { return t.feat & kVarFeatMask; }
// What a launch of `t` asks the dispatch for.
inline TileVariant tile_variant(const TileArgs& t, bool timing) {
  return TileVariant{t.lds_tables != 0, timing, tile_feat(t), tile_kernel_kind(t, timing) == kTileKernelProd};
}
// The instantiation evaluate_tiles_kernel<ldst, timing, feat, prod> a request resolves to: several
// requests share one (the production shape has LDS tables and no clocks; an NFA element takes the
// every-family kernel, clocks or not; the wave scan exists for the label / container set with LDS
// tables and no clocks; the clocks keep the C2 / C3 / C4 family sets with LDS tables and run every
// other set on the every-family kernel). tile_fn picks the kernel by this function's result alone.
constexpr TileVariant tile_resolve(const TileVariant& v) {
  const uint32_t fam = v.feat & kFeatAll;
  if (v.prod) return TileVariant{true, false, kFeatLbl | kFeatCtr | (v.feat & kFeatRng), true};
  if (v.feat & kFeatNfa) return TileVariant{v.ldst, false, kFeatAll | kFeatNfa, false};
  if ((v.feat & kFeatRng) && v.ldst && !v.timing && fam == (kFeatLbl | kFeatCtr))
    return TileVariant{true, false, kFeatLbl | kFeatCtr | kFeatRng, false};
  if (v.timing) {
    const bool own = v.ldst && (fam == kFeatImg || fam == (kFeatImg | kFeatGrp) || fam == (kFeatLbl | kFeatCtr));
    return TileVariant{v.ldst, true, own ? fam : kFeatAll, false};
  }
  return TileVariant{v.ldst, false, fam, false};
}

// One launch of the tile kernel over chunks t.chunk[0..nchunk). t: host copy (launch geometry);
// d_t: the same TileArgs resident in device memory (read by the kernel).
hipError_t launch_evaluate_tiles(const EvalArgs& a, const TileArgs& t, const TileArgs* d_t, const TileDesc* d_desc,
                                 uint32_t grid, hipStream_t s);
// Requests that do not fit the LDS capacities even alone (d_overflow: [count, request indices...],
// host-built with the descriptors): classified into HBM, then walked sequentially per request.
hipError_t launch_overflow(const EvalArgs& a, const TileArgs* d_t, const uint32_t* d_overflow, uint32_t n_overflow,
                           hipStream_t s);

// The NFA elements of a pass (kwdev.hpp DevNfa): every label value under its key's chain and every
// image reference under the registry / tag / image chains, one thread per entity, a Pike VM per
// element with its lists in `scratch` (words_per_thread u32 per thread of the grid: the largest
// program's nfa_scratch_words, then room for a normalised image reference of subj_bytes).
struct NfaPass {
  uint16_t* lv;   // [nlabels][nlv]
  uint16_t* img;  // [nctrs][nim]
  uint32_t* scratch;
  uint64_t words_per_thread;
  uint32_t nfa_words, subj_bytes;
  uint32_t nlv, nim;
  uint64_t nlabels, nctrs;
  uint32_t do_lv, do_img;
};
// Bulk path (kw_validate_host): a chunk's column ranges arrive in one H2D copy, packed, and this
// kernel moves each range to its place in the batch's device image (one copy per chunk instead of
// one per column: a pinned H2D copy costs ~9.6 us on its own, profiles/r05_bulk_copies.txt).
// src_off == dst_off (mod 16), so the body moves 16-byte words.
constexpr uint32_t kMaxScatterSegs = 24;
struct ScatterSeg {
  uint64_t dst_off, src_off, bytes;
};
struct ScatterArgs {
  uint8_t* dst;
  const uint8_t* src;
  uint32_t nseg;
  ScatterSeg seg[kMaxScatterSegs];
};
hipError_t launch_scatter(const ScatterArgs& a, hipStream_t s);

hipError_t launch_nfa_classify(const EvalArgs& a, const TileArgs* d_t, const NfaPass& np, uint32_t threads, hipStream_t s);
// threads of the NFA pass's grid for `items` entities within a scratch budget
uint32_t nfa_threads(uint64_t items, uint64_t words_per_thread);

}  // namespace kw
