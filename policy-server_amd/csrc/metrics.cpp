// metrics.cpp — batched policy-evaluation metrics (metrics.hpp).
#include "metrics.hpp"

#include <algorithm>

#include "outcomes.hpp"

namespace kw {

constexpr uint64_t Metrics::kBounds[];

namespace {

// Prometheus label value escaping: backslash, double quote, newline.
void put_label(std::string* o, bool first, const char* key, std::string_view v) {
  if (!first) o->push_back(',');
  o->append(key);
  o->append("=\"");
  for (char c : v) {
    if (c == '\\') o->append("\\\\");
    else if (c == '"') o->append("\\\"");
    else if (c == '\n') o->append("\\n");
    else o->push_back(c);
  }
  o->push_back('"');
}

}  // namespace

// The label set of one series: the policy's attributes, the row's, and the outcome of the word
// (outcomes.hpp outcome_code). The one place that knows the reference's attribute keys and their
// order; record and add_outcomes both build their keys here.
std::string Metrics::label_set(const Env& env, const Batch& b, uint64_t row, int32_t policy, uint32_t outcome, int origin) {
  const PolicyRec& P = env.pol[(size_t)policy];
  std::string key;
  if (outcome == KW_OUT_INIT_ERROR) {
    // PolicyInitializationError (metrics.rs:125-140; service.rs:78-84): the counter only
    put_label(&key, true, "policy_name", P.id);
    put_label(&key, false, "initialization_error", P.init_message);
    return key;
  }
  const bool raw = (b.req_flags[row] & KW_REQ_RAW) != 0;
  const char* mode = P.mode == KW_MODE_MONITOR ? "monitor" : "protect";  // config.rs:296-302
  // a bypass (service.rs:45-58) is accepted, not mutated, no error code; else the vanilla response
  // (service.rs:97-105), error code 500 for reject(uid, rhai error, 500): outcome_code
  const bool accepted = (outcome & KW_OUT_ACCEPTED) != 0, mutated = (outcome & KW_OUT_MUTATED) != 0;
  put_label(&key, true, "policy_name", P.id);
  put_label(&key, false, "policy_mode", mode);
  if (raw) {  // RawPolicyEvaluation (metrics.rs:96-123)
    put_label(&key, false, "accepted", accepted ? "true" : "false");
    put_label(&key, false, "mutated", mutated ? "true" : "false");
  } else {  // PolicyEvaluation (metrics.rs:49-94)
    put_label(&key, false, "resource_kind", row < b.rkind.n() ? b.rkind.at(row) : std::string_view());
    put_label(&key, false, "resource_request_operation", b.op.at(row));
    put_label(&key, false, "accepted", accepted ? "true" : "false");
    put_label(&key, false, "mutated", mutated ? "true" : "false");
    put_label(&key, false, "request_origin", origin == KW_ORIGIN_AUDIT ? "audit" : "validate");
    if (b.req_flags[row] & KW_REQ_HAS_NAMESPACE) put_label(&key, false, "resource_namespace", b.ns.at(row));
  }
  if (outcome & KW_OUT_ERROR_500) put_label(&key, false, "error_code", "500");
  return key;
}

// n data points of one series (the caller holds mu_).
void Metrics::add_locked(const std::string& key, uint32_t outcome, uint64_t n, uint64_t latency_ms) {
  total_[key] += n;
  if (outcome == KW_OUT_INIT_ERROR) return;
  Hist& h = latency_[key];
  const size_t k = std::lower_bound(kBounds, kBounds + kNB, latency_ms) - kBounds;  // first bound >= latency
  h.bucket[k] += n;
  h.sum += n * latency_ms;
  h.count += n;
}

void Metrics::record(const Env& env, const Batch& b, uint64_t row, int32_t policy, uint32_t v, int origin,
                     uint64_t latency_ms) {
  if (policy < 0 || (size_t)policy >= env.nvisible || row >= b.n) return;
  const uint32_t outcome = outcome_code(v);
  const std::string key = label_set(env, b, row, policy, outcome, origin);
  std::lock_guard<std::mutex> g(mu_);
  add_locked(key, outcome, 1, latency_ms);
}

bool Metrics::add_outcomes(const Env& env, const Batch& b, const int32_t* policies, uint32_t npol, int origin,
                           uint64_t latency_ms, const uint64_t* first_row, uint32_t ngroups, const uint64_t* counts) {
  for (uint32_t g = 0; g < ngroups; ++g)
    if (first_row[g] >= b.n) return false;
  std::lock_guard<std::mutex> lock(mu_);
  for (uint32_t g = 0; g < ngroups; ++g)
    for (uint32_t k = 0; k < (uint32_t)KW_OUT_N; ++k) {
      const uint64_t* n = counts + ((size_t)g * KW_OUT_N + k) * npol;
      for (uint32_t c = 0; c < npol; ++c) {
        if (!n[c] || policies[c] < 0 || (size_t)policies[c] >= env.nvisible) continue;
        add_locked(label_set(env, b, first_row[g], policies[c], k, origin), k, n[c], latency_ms);
      }
    }
  return true;
}

std::string Metrics::render() const {
  std::lock_guard<std::mutex> g(mu_);
  std::string o;
  o.append("# TYPE kubewarden_policy_evaluations_total counter\n");
  for (const auto& [k, n] : total_) {
    o.append("kubewarden_policy_evaluations_total{").append(k).append("} ").append(std::to_string(n)).push_back('\n');
  }
  o.append("# TYPE kubewarden_policy_evaluation_latency_milliseconds histogram\n");
  for (const auto& [k, h] : latency_) {
    uint64_t cum = 0;
    for (size_t i = 0; i <= kNB; ++i) {
      cum += h.bucket[i];
      o.append("kubewarden_policy_evaluation_latency_milliseconds_bucket{").append(k).append(",le=\"");
      o.append(i < kNB ? std::to_string(kBounds[i]) : std::string("+Inf")).append("\"} ");
      o.append(std::to_string(cum)).push_back('\n');
    }
    o.append("kubewarden_policy_evaluation_latency_milliseconds_sum{").append(k).append("} ");
    o.append(std::to_string(h.sum)).push_back('\n');
    o.append("kubewarden_policy_evaluation_latency_milliseconds_count{").append(k).append("} ");
    o.append(std::to_string(h.count)).push_back('\n');
  }
  return o;
}

void Metrics::reset() {
  std::lock_guard<std::mutex> g(mu_);
  total_.clear();
  latency_.clear();
}

}  // namespace kw
