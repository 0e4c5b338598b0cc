// pools.cpp — the pools' singletons and the parallel host copies (pools.hpp).
#include "pools.hpp"

#include <algorithm>
#include <cstring>
#include <thread>

#include "knobs.hpp"

namespace kw {

StreamPool::StreamPool() : on(Knobs::on<KW_STREAM_POOL>()) {}

HostWorkers::HostWorkers() {
  const int e = Knobs::num<KW_HOST_THREADS>();
  unsigned n = e ? (unsigned)e : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  for (unsigned i = 1; i < n; ++i) std::thread([this] { loop(); }).detach();
}

BlockPool& dev_pool() {
  static BlockPool* p = new BlockPool(false);  // process lifetime (blocks outlive every batch)
  return *p;
}
BlockPool& host_pool() {
  static BlockPool* p = new BlockPool(true);
  return *p;
}

StreamPool& stream_pool() {
  static StreamPool* p = new StreamPool;  // process lifetime, like the block pools
  return *p;
}

void parallel_copy(void* dst, const void* src, size_t bytes) {
  constexpr size_t kMin = (size_t)8 << 20;
  if (bytes < kMin) {
    memcpy(dst, src, bytes);
    return;
  }
  const size_t nt = std::min<size_t>(16, std::max<size_t>(1, std::min<size_t>(std::thread::hardware_concurrency(), bytes / (kMin / 2))));
  std::vector<std::thread> th;
  for (size_t t = 0; t < nt; ++t) {
    const size_t a = bytes * t / nt, e = bytes * (t + 1) / nt;
    th.emplace_back([=] { memcpy((uint8_t*)dst + a, (const uint8_t*)src + a, e - a); });
  }
  for (auto& x : th) x.join();
}

void parallel_copy_segs(const std::vector<CopySeg>& segs) {
  constexpr size_t kTask = (size_t)1 << 20;
  std::vector<CopySeg> tasks;
  for (const CopySeg& c : segs)
    for (size_t a = 0; a < c.bytes; a += kTask)
      tasks.push_back({(uint8_t*)c.dst + a, (const uint8_t*)c.src + a, std::min(kTask, c.bytes - a)});
  HostWorkers::get().run(tasks.size(), [&](size_t i) { memcpy(tasks[i].dst, tasks[i].src, tasks[i].bytes); });
}

}  // namespace kw
