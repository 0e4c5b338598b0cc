// reports.hpp — launch interface of the report kernels (reports.hip), which read the verdict words
// the hot path (kernels.hpp) wrote.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "digest.hpp"
#include "members.hpp"
#include "messages.hpp"
#include "outcomes.hpp"
#include "packed.hpp"
#include "patches.hpp"
#include "responses.hpp"
#include "summary.hpp"

namespace kw {

// Bulk path, packed output (kw_validate_host_packed; the format and its arithmetic: packed.hpp): a
// chunk's verdict words into bit-planes, absolute per-row exception offsets and the exception words,
// behind the chunk's kernels on the same stream. Five launches, none waiting on another workgroup:
//   codes    a lane per column, a wave per item (row, 64-column group) or per 64 / npol rows where
//            npol <= 32: two ballots give the planes, the popcount of their AND the item's count
//   sums     per-workgroup sums of the counts        scan   one workgroup over the sums, seeded with
//   bases    the counts into absolute bases, exc_off        tot[0] (the chunks before); tot[1] = total
//   scatter  each escaped lane's word at its item's base + its rank in the item, less tot[0]
// All pointers at the chunk's first row / item; rows x G = nitems.
struct PackArgs {
  const uint32_t* words;  // [rows][npol]
  const uint32_t* dict;   // [npol][3]
  uint64_t* planes;       // [nitems][2]
  uint32_t* ibase;        // [nitems]: counts, then absolute bases
  uint32_t* exc_off;      // [rows], and [rows] = the total after the chunk
  uint32_t* bsum;         // [ceil(nitems / kScanBlock)]
  uint32_t* tot;          // [2]: the total before the chunk (read), after it (written)
  uint32_t* exc;          // the chunk's exception words
  uint32_t exc_cap;
  uint32_t npol, G, nitems;
};
hipError_t launch_pack(const PackArgs& a, hipStream_t s);

// The summary form (kw_batch_summary, kw_validate_host_summary; the form and the geometry:
// summary.hpp): a streaming pass over row-major verdict words, each read once. Two launches:
//   summary  a lane keeps one column for the whole kernel, a wave one column group (grid.y) and the
//            units of rows its index strides to. The flag and status counters are plain adds in
//            registers; the 17 reason buckets a per-wave LDS table [lane][bucket] of odd row stride
//            (lanes with the same reason hit distinct banks; KW_SUM_LDS=0 builds the compare-and-add
//            form in registers: profiles/r10_summary.txt has the two side by side). The planes come
//            from two ballots a round, lane j keeping round j's, stored 16 bytes a row after a unit.
//            The waves of a workgroup, and the lanes that share a column where npol <= 32, combine in
//            LDS; the workgroup writes one u32 partial block [columns][KW_SUM_N]. No global atomics.
//   totals   a workgroup per column sums the partial blocks in eight slices side by side, then one
//            thread per counter adds the slices in a fixed order into the running u64 totals `tot`:
//            ordered by the stream, so the chunks of a bulk pass accumulate into it.
// All pointers at the launch's first row; `part` holds summary_part_bytes(rows, npol).
struct SumArgs {
  const uint32_t* words;  // [rows][npol]
  uint64_t* planes;       // [rows][G][2], or nullptr: counters only
  uint32_t* part;         // the workgroups' partial blocks
  uint64_t* tot;          // [npol][KW_SUM_N], added to
  uint64_t rows;
  uint32_t npol;
};
hipError_t launch_summary(const SumArgs& a, hipStream_t s);
// Bytes of SumArgs::part for launches of up to `rows` rows on the current device.
size_t summary_part_bytes(uint64_t rows, uint32_t npol);

// kw_batch_verdict_rows: out[i][0..row_words) = words[rows[i]][0..row_words) for n device rows.
struct GatherArgs {
  const uint32_t* words;
  const uint64_t* rows;
  uint32_t* out;
  uint64_t n;
  uint32_t row_words;
};
hipError_t launch_gather_rows(const GatherArgs& a, hipStream_t s);

// The grouped outcome count (kw_batch_outcomes; the outcome, the sort and the unit table:
// outcomes.hpp): one pass over the verdict words, gathered by whole rows in group order. A wave takes
// one unit (one group's run of at most kOutUnitRows sorted entries), grid.y the column groups of 64;
// a lane keeps one column (pack_geom's w lanes a row, ipi rows a load where npol <= 32), kOutLoads row
// loads in flight and the nine outcome counters in registers by compare-and-add. After its unit the
// wave adds the counters some lane holds to the u64 table with relaxed agent-scope vector atomics:
// one outcome's adds are contiguous, the lanes that share a column are summed by shuffles first.
// No LDS memory, no fence: the stream orders the table's zeroing before and its read-back after. Integer
// adds, so the table does not depend on the order in which the waves arrive.
struct OutcomeArgs {
  const uint32_t* words;  // [rows][npol], device-row order
  const uint32_t* order;  // device rows sorted by group (every entry < rows)
  const OutUnit* units;   // this launch's units (first / n index `order`)
  uint64_t* table;        // [groups of the range][KW_OUT_N][npol], added to
  uint32_t nunits, npol;
  uint32_t g0;            // the range's first group: unit group g counts into table row g - g0
};
hipError_t launch_outcomes(const OutcomeArgs& a, hipStream_t s);

// The violation digest (kw_batch_digest; the key, the hash and the table: digest.hpp): three launches
// over one column range [c0, c1) of the verdict words, none waiting on another workgroup.
//   count    the words walked with the summary's geometry (a lane keeps a column, grid.y the column
//            groups of 64, a wave strides over units of kDigestRounds rounds). Findings are sparse: a
//            lane that holds one reads its key bytes from the HBM columns through the offset arrays
//            (plain vector loads), hashes (column, class, key) and holds the findings of its column's
//            four busiest tags in registers; an evicted run goes to its slot: the tag claimed by a 64-bit compare-and-swap, the
//            count by a 64-bit add, the representative by a 64-bit unsigned max that a plain load
//            skips when it cannot win. Wide findings append their pair index through one counter.
//   verify   a launch of its own, so every representative is final: each finding finds its slot
//            again and compares its column, class and key bytes with the representative's; on a
//            mismatch it goes to the bounded leftover list and its slot's count drops by one.
//   gather   the live slots into records, in any order (the host sorts).
// Relaxed agent-scope vector atomics and plain vector stores only; the stream orders the launches, the
// zeroing before and the read-back after. Integer adds and a max: the table's final state does not
// depend on the order in which the waves arrive.
struct DigestArgs {
  const uint32_t* words;  // [rows][npol], device-row order
  DigestCols cols;        // the device columns (device rows)
  const uint32_t* d2b;    // the batch row of each device row, nullptr: the same
  const uint32_t* b2d;    // and the reverse
  DigestSlot* table;
  DigestHead* head;
  uint64_t* wide;         // [wide_cap] device pair indices
  DigestLeft* left;       // [left_cap]
  kw_digest_rec* recs;    // [rec_cap] (gather)
  uint64_t nslots, wide_cap, rec_cap;
  uint32_t left_cap, hash_bits;
  uint32_t npol, c0, c1;
  uint32_t loaded;        // string columns (bits of Str) that are resident
};
hipError_t launch_digest_count(const DigestArgs& a, hipStream_t s);
hipError_t launch_digest_verify(const DigestArgs& a, hipStream_t s);
hipError_t launch_digest_gather(const DigestArgs& a, hipStream_t s);

// The digest's drill-down (kw_batch_digest_members; the table, the probe and the order: members.hpp):
// two launches over the verdict words, none waiting on another workgroup.
//   check    one thread per slot of the selection table: a slot that names a group compares the
//            pass's word at its representative with the record's word and raises head->bad when they
//            differ (a record of another pass). Per slot and not per record, so the table is all the
//            device needs of the record list.
//   walk     the words walked with the digest's geometry (digest_lane: a lane keeps a column, grid.y
//            the column groups of 64, a unit's loads in flight before the first is used). A lane
//            holds its column's mask of selected classes in a register: a finding of another class
//            never touches its key bytes, and a wave none of whose columns has a named group leaves
//            at once. A finding that passes hashes its key and probes (members_find). The members of
//            a unit take their places in the list through one add per wave (a scan of the lanes'
//            counts, one lane adds the total), and write (group, batch row, word) while the place is
//            below list_cap; a lane's run of members of one group adds to that group's count once.
//            Counting goes on past list_cap, so the counts stay exact.
// Relaxed agent-scope vector atomics and plain vector stores only, no LDS; the stream orders the
// launches, the zeroing before and the read-back after. Integer adds: the counts do not depend on
// the order in which the waves arrive, the list's order does (the host sorts it).
struct MembersArgs {
  const uint32_t* words;    // [rows][npol], device-row order
  DigestCols cols;          // the device columns (device rows)
  const uint32_t* d2b;      // the batch row of each device row, nullptr: the same
  const MemberSlot* table;  // [nslots], rep_row in device rows
  const uint64_t* colmask;  // [npol] members_class_bit masks
  uint64_t* counts;         // [ngroups], added to
  MemberEntry* list;        // [max(list_cap, 1)]
  MembersHead* head;
  uint64_t nslots, list_cap;
  uint32_t hash_bits, npol;
  uint32_t loaded;          // string columns (bits of Str) that are resident
};
hipError_t launch_members_check(const MembersArgs& a, hipStream_t s);
hipError_t launch_members_walk(const MembersArgs& a, hipStream_t s);

// The messages of chosen findings (kw_batch_messages; the pieces, the windows and the settings
// table: messages.hpp): three steps over one round of n items, ordered by the stream.
//   len      one lane per item: the pass's word at (device row, col), message_pieces, the length,
//            the word when asked for, the mark of an item left to the host; a message that quotes a
//            column that is not resident raises head->missing.
//   scan     the exclusive scan of the lengths into off[i] = base + the lengths before i (u64),
//            off[n] the round's end, in the pack kernels' three steps: sums (a workgroup a tile of
//            kMsgScanTile lengths, its total), bases (one workgroup scans the tiles' totals in
//            place), scan (a workgroup a tile again, from its base); wave scans by shuffles, the
//            waves' totals through LDS. One workgroup over all lengths took 6.9 ms for 11.6 M items
//            (profiles/r16_messages.txt).
//   write    a workgroup of one wave owns 64 consecutive items, so its output is one contiguous byte
//            range. It walks the range in windows of `window` bytes of LDS that start at multiples
//            of 16: each lane runs message_pieces again and copies the part of its message inside
//            the window (msg_clip, msg_copy_window: LDS byte and dword writes); after the barrier
//            the wave stores the window with aligned 16-byte global stores, the range's unaligned
//            head and tail in single bytes, and nothing outside [off[i0], off[i0 + 64)). Byte g of
//            the call's text lies at text[g - text_base], text_base a multiple of 16.
// Plain vector loads and stores and relaxed agent-scope vector atomics (the counters of head) only.
struct MessagesHead {
  uint64_t windows, spanning;  // windows written; messages that touched more than one
  uint32_t missing, pad;
};
constexpr uint32_t kMsgScanThreads = 1024, kMsgScanTile = 4096;
struct MessagesArgs {
  const uint32_t* words;    // [rows][npol], device-row order
  MsgCols cols;             // the device columns (device rows) and the container names
  const uint8_t* settings;  // the pass's settings table (msg_settings)
  const uint32_t* drow;     // [n] device rows
  const uint32_t* col;      // [n]
  uint32_t* len;            // [n]
  uint32_t* out_words;      // [n] or nullptr
  uint8_t* mark;            // [n] 1: left to the host
  uint64_t* off;            // [n + 1]
  uint64_t* sums;           // [ceil(n / kMsgScanTile)]: the tiles' totals, then their bases
  uint8_t* text;
  MessagesHead* head;
  uint64_t base, text_base;
  uint32_t n, npol, window;
};
hipError_t launch_messages_len(const MessagesArgs& a, hipStream_t s);
hipError_t launch_messages_scan(const MessagesArgs& a, hipStream_t s);
hipError_t launch_messages_write(const MessagesArgs& a, hipStream_t s);

// The AdmissionResponse bodies of chosen pairs (kw_batch_responses; the forms, the parts, the
// escaping and the table: responses.hpp): the steps of the messages over one round of n items.
//   len      one lane per item: rsp_item gives the form or leaves the item to the host, rsp_measure
//            walks the item's parts (the head, the message, two per cause, the tail) and sums their
//            escaped lengths; the members' words of a group are read from the same row of the
//            pass. The pieces that grew by escaping are counted into head->escaped.
//   scan     the messages' scan kernels over these lengths (launch_messages_scan on a MessagesArgs
//            that names len, off, sums, base and n).
//   write    messages_write_kernel's walk: a workgroup of one wave owns 64 consecutive items and
//            their contiguous byte range, in windows of `window` bytes of LDS. A lane whose response
//            touches the window walks its parts again (rsp_render_window) and writes the bytes
//            inside it: pieces without escapes by the dword copy, escaped ones byte by byte, an
//            escape cut by the window's edge in part. The window leaves by aligned 16-byte stores.
// Plain vector loads and stores and relaxed agent-scope vector atomics (the counters of head) only.
struct ResponsesHead {
  uint64_t windows, spanning, escaped;
  uint32_t missing, pad;
};
struct ResponsesArgs {
  const uint32_t* words;    // [rows][npol], device-row order
  MsgCols cols;             // the device columns (device rows) and the container names
  DigestStr uid;            // the uid column, device rows
  const uint8_t* settings;  // the responses' table (rsp_settings)
  const uint32_t* drow;     // [n] device rows
  const uint32_t* col;      // [n]
  uint32_t* len;            // [n]
  uint32_t* out_words;      // [n] or nullptr
  uint8_t* mark;            // [n] 1: left to the host
  const uint64_t* off;      // [n + 1] (the scan's)
  uint8_t* text;
  ResponsesHead* head;
  uint64_t text_base;
  uint32_t n, npol, window;
};
hipError_t launch_responses_len(const ResponsesArgs& a, hipStream_t s);
hipError_t launch_responses_write(const ResponsesArgs& a, hipStream_t s);

// The JSONPatch of accepted mutations (kw_batch_patches; the walk, the table and the base64 layer:
// patches.hpp): the frame of the responses (`r`: the items, the lengths, the scan's offsets, the
// text, the head; its cols and uid are not read), the columns a patch is cut from and the form.
//   len      one lane per item: patch_item leaves the item to the host or not, patch_measure walks
//            the row's containers and gives the length of the ops text, the response form adds the
//            envelope and turns the ops' length into its base64's.
//   scan     the messages' scan kernels, as for the responses.
//   write    the responses' walk over windows of LDS (window_store). In the ops form a lane walks
//            its item again and keeps the bytes inside the window. In the response form the
//            window's base64 characters need the raw bytes under their quads: the lane renders
//            those into a second LDS region (3/4 of the window and 8 bytes a lane, each lane a
//            place of its own) and encodes from there; its span is cut to whole quads counted from
//            the start of the item's base64 text, so a quad that straddles two windows is encoded
//            from the same three bytes both times.
// Plain vector loads and stores and relaxed agent-scope vector atomics (the counters of head) only.
struct PatchesArgs {
  ResponsesArgs r;
  PatchCols c;    // device rows
  uint32_t form;  // KW_PATCH_OPS / KW_PATCH_RESPONSE
};
hipError_t launch_patches_len(const PatchesArgs& a, hipStream_t s);
hipError_t launch_patches_write(const PatchesArgs& a, hipStream_t s);

}  // namespace kw
