// rounds.hpp — the rounds that kw_batch_responses and kw_batch_patches share (responses.cpp): the
// items in rounds of KW_MESSAGES_CHUNK, each round its lengths, their scan (the messages' scan
// kernels) and its text, the offsets, the words and the host marks back through a pooled block, the
// text by direct DMA into page-locked memory or through a bounce block, KW_E_NOSPACE with bytes,
// nhost and all of off exact. The caller has opened the frame, uploaded its side columns and filled
// the column views of `a`; the two launches are its own.
#pragma once
#include <chrono>
#include <functional>
#include <vector>

#include "lastpass.hpp"
#include "reports.hpp"

namespace kw {

using RoundLaunch = std::function<hipError_t(const ResponsesArgs&, hipStream_t)>;
struct RoundsCall {
  RoundLaunch len, write;
  const char* what;     // the name in the KW_BULK_DEBUG line
  uint64_t* stats;      // [6]: rounds, windows, spanning, host items, (the caller's), escaped pieces
  double side_ms = 0;   // what the caller spent on side columns
  std::chrono::steady_clock::time_point t_start;
};
// rows and cols are checked against the pass by the caller; n > 0.
int response_rounds(LastPass& F, const std::vector<uint64_t>& table, ResponsesArgs a, const uint64_t* rows, const uint32_t* cols,
                    size_t n, kw_responses* out, const RoundsCall& call);
// The checks of kw_responses' pointers.
bool responses_out_ok(const kw_responses* out, const uint64_t* rows, const uint32_t* cols, size_t n);
// The uid column to the device on stream s (DeviceBatch::uids), device-row order.
int upload_uids(kw_batch* kb, hipStream_t s);

}  // namespace kw
