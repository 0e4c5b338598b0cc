// pools.hpp — process-lifetime helpers of the host engine: caching allocators, the stream / event
// pool, the host worker pool and the parallel copies built on it (pools.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace kw {

// Caching allocators for device memory and pinned host staging: a micro-batch front evaluates
// thousands of small batches per second, and hipMalloc / hipHostMalloc per batch would dominate.
// Blocks are kept per (device, size class) up to max_cached() bytes per pool.
struct BlockPool {
  bool host;
  std::mutex m;
  std::map<std::pair<int, size_t>, std::vector<void*>> free;
  size_t cached = 0;
  // cached bytes: device 32 GiB (of 288), pinned host 16 GiB — the bulk path's per-call blocks
  // (bounce, ring, descriptors) and a re-uploaded batch's image come back from the cache
  size_t max_cached() const { return host ? (size_t)16 << 30 : (size_t)32 << 30; }
  explicit BlockPool(bool h) : host(h) {}
  // size classes: 4 KiB, then eight steps per power of two (<= 12.5 % slack: C5's 3.6 GB image
  // took a 4 GiB block before)
  static size_t cls(size_t n) {
    if (n <= 4096) return 4096;
    size_t p = 4096;
    while (p * 2 < n) p <<= 1;  // p < n <= 2p
    const size_t step = p / 8;
    return (n + step - 1) / step * step;
  }
  hipError_t alloc(int dev, size_t n, void** p) {
    const size_t c = cls(n);
    {
      std::lock_guard<std::mutex> g(m);
      auto& v = free[{dev, c}];
      if (!v.empty()) {
        *p = v.back();
        v.pop_back();
        cached -= c;
        return hipSuccess;
      }
    }
    return host ? hipHostMalloc(p, c, hipHostMallocDefault) : hipMalloc(p, c);
  }
  void release(int dev, void* p, size_t n) {
    if (!p) return;
    const size_t c = cls(n);
    std::lock_guard<std::mutex> g(m);
    if (cached + c > max_cached()) {
      (void)(host ? hipHostFree(p) : hipFree(p));
      return;
    }
    free[{dev, c}].push_back(p);
    cached += c;
  }
};

// Non-blocking streams and timing-free events handed back for reuse, per device: creating a
// stream costs host time on the order of a tenth of a millisecond, and a bulk pass used three.
// A stream returns here drained (its owner synchronized it). KW_STREAM_POOL=0: A/B knob.
struct StreamPool {
  std::mutex m;
  std::map<int, std::vector<hipStream_t>> streams;
  std::map<int, std::vector<hipEvent_t>> events;
  const bool on;
  StreamPool();
  hipError_t get(int dev, hipStream_t* s) {
    if (on) {
      std::lock_guard<std::mutex> g(m);
      auto& v = streams[dev];
      if (!v.empty()) {
        *s = v.back();
        v.pop_back();
        return hipSuccess;
      }
    }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  }
  void put(int dev, hipStream_t s) {
    if (!s) return;
    if (!on) {
      (void)hipStreamDestroy(s);
      return;
    }
    std::lock_guard<std::mutex> g(m);
    streams[dev].push_back(s);
  }
  hipError_t get(int dev, hipEvent_t* e) {
    if (on) {
      std::lock_guard<std::mutex> g(m);
      auto& v = events[dev];
      if (!v.empty()) {
        *e = v.back();
        v.pop_back();
        return hipSuccess;
      }
    }
    return hipEventCreateWithFlags(e, hipEventDisableTiming);
  }
  void put(int dev, hipEvent_t e) {
    if (!e) return;
    if (!on) {
      (void)hipEventDestroy(e);
      return;
    }
    std::lock_guard<std::mutex> g(m);
    events[dev].push_back(e);
  }
};

// Persistent host workers for the bulk path (kw_validate_host): a parallel-for over many short
// tasks (copy segments, tile ranges) without starting threads per call. The caller runs tasks too.
// Each call is a Job on the caller's stack; a worker joins it under the lock (users + 1) and the
// caller returns only when every task is done and every worker that joined has left, so no worker
// ever sees another call's counters or a finished call's function.
class HostWorkers {
 public:
  static HostWorkers& get() {
    static HostWorkers* w = new HostWorkers();  // process lifetime (workers park on a condition)
    return *w;
  }
  // fn(i) for every i in [0, n), spread over the workers and the caller; returns when all are done
  // A single task runs inline on the caller: no lock, no wake-up (kwhost's small micro-batches plan
  // one tile range per pass, and its pipeline workers must not serialise on run_m_ for that).
  void run(size_t n, const std::function<void(size_t)>& fn) {
    if (n == 0) return;
    if (n == 1) {
      fn(0);
      return;
    }
    std::lock_guard<std::mutex> one(run_m_);  // one parallel-for at a time
    Job job;
    job.fn = &fn;
    job.n = n;
    {
      std::lock_guard<std::mutex> g(m_);
      job_ = &job;
      ++gen_;
    }
    cv_.notify_all();
    const size_t mine = job.work();
    std::unique_lock<std::mutex> g(m_);
    job_ = nullptr;  // no worker joins after this
    job.done += mine;
    done_cv_.wait(g, [&] { return job.done == job.n && job.users == 0; });
  }

 private:
  struct Job {
    const std::function<void(size_t)>* fn = nullptr;
    size_t n = 0;
    std::atomic<size_t> next{0};
    size_t done = 0;     // tasks finished (under m_)
    unsigned users = 0;  // workers inside work() (under m_)
    size_t work() {
      size_t k = 0;
      for (size_t i; (i = next.fetch_add(1)) < n; ++k) (*fn)(i);
      return k;
    }
  };
  HostWorkers();  // KW_HOST_THREADS - 1 workers (pools.cpp)
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      Job* j = nullptr;
      {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [&] { return gen_ != seen && job_ != nullptr; });
        seen = gen_;
        j = job_;
        ++j->users;
      }
      const size_t mine = j->work();
      std::lock_guard<std::mutex> g(m_);
      j->done += mine;
      --j->users;
      if (j->done == j->n && j->users == 0) done_cv_.notify_all();
    }
  }
  std::mutex m_, run_m_;
  std::condition_variable cv_, done_cv_;
  Job* job_ = nullptr;
  uint64_t gen_ = 0;
};

// Copies of several (dst, src, bytes) segments cut into ~1 MB tasks on the host workers.
struct CopySeg {
  void* dst;
  const void* src;
  size_t bytes;
};

BlockPool& dev_pool();
BlockPool& host_pool();
StreamPool& stream_pool();

// Move-only owners of what a call takes from the pools: it goes back when the owner dies.
// The owner's user drains the streams that touch a block or an event before that (bulk.cpp Res).
struct BlockLease {
  BlockPool* pool = nullptr;
  int dev = -1;
  void* p = nullptr;
  size_t bytes = 0;
  BlockLease() = default;
  BlockLease(BlockLease&& o) noexcept : pool(o.pool), dev(o.dev), p(o.p), bytes(o.bytes) { o.p = nullptr; }
  ~BlockLease() { reset(); }
  // a block of n bytes of P in place of the one held
  hipError_t alloc(BlockPool& P, int d, size_t n) {
    reset();
    pool = &P, dev = d, bytes = n;
    return P.alloc(d, n, &p);
  }
  void reset() {
    if (p) pool->release(dev, p, bytes);
    p = nullptr;
  }
};

struct StreamLease {
  int dev = -1;
  hipStream_t s = nullptr;
  StreamLease() = default;
  StreamLease(StreamLease&& o) noexcept : dev(o.dev), s(o.s) { o.s = nullptr; }
  ~StreamLease() { stream_pool().put(dev, s); }
  hipError_t get(int d) {
    dev = d;
    return stream_pool().get(d, &s);
  }
};

struct EventLease {
  int dev = -1;
  std::vector<hipEvent_t> ev;
  EventLease() = default;
  EventLease(EventLease&& o) noexcept : dev(o.dev), ev(std::move(o.ev)) { o.ev.clear(); }
  ~EventLease() {
    for (hipEvent_t e : ev) stream_pool().put(dev, e);
  }
  // n events; on an error the ones already taken stay owned
  hipError_t get(int d, size_t n) {
    dev = d;
    ev.assign(n, nullptr);
    for (hipEvent_t& e : ev)
      if (hipError_t rc = stream_pool().get(d, &e)) return rc;
    return hipSuccess;
  }
  hipEvent_t operator[](size_t i) const { return ev[i]; }
};

// Host copy spread over up to 16 threads for large buffers (staging fills and verdict read-back:
// one thread moves ≈ 10 GB/s, the host's memory system several times that).
void parallel_copy(void* dst, const void* src, size_t bytes);
void parallel_copy_segs(const std::vector<CopySeg>& segs);

}  // namespace kw
