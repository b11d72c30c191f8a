// sdsj_stage_pool.h -- an engine's staging threads (standard library only).
//
// Kept across calls: starting and joining 7 threads per parallel_for cost as much as the parallel
// memcpy saved (submit 1.29 ms serial vs 1.44 ms with 8 fresh threads per 256-image batch at 16
// DataLoader workers, profiles/r06_f1_stage_threads.jsonl).  One parallel_for at a time, from one
// thread at a time: an engine takes one host call at a time (include/sdsj.h), and the pool has one
// owner.  Worker k runs part k of the current call's range and the caller runs part 0.
#pragma once
#include <stdint.h>

#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace sdsj {

struct StagePool {
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable go, done;
  std::function<void(int, int)> fn;
  int n = 0, nt = 0, left = 0;
  uint64_t gen = 0;
  bool stop = false;
  explicit StagePool(int workers) {
    for (int k = 1; k <= workers; k++) th.emplace_back([this, k] { run(k); });
  }
  ~StagePool() {
    {
      std::lock_guard<std::mutex> l(m);
      stop = true;
    }
    go.notify_all();
    for (auto& t : th) t.join();
  }
  void run(int k) {
    uint64_t seen = 0;
    for (;;) {
      std::function<void(int, int)> f;
      int a = 0, b = 0;
      {
        std::unique_lock<std::mutex> l(m);
        go.wait(l, [&] { return stop || gen != seen; });
        if (stop) return;
        seen = gen;
        if (k >= nt) continue;
        f = fn;
        a = (int)((int64_t)n * k / nt);
        b = (int)((int64_t)n * (k + 1) / nt);
      }
      f(a, b);
      std::lock_guard<std::mutex> l(m);
      if (--left == 0) done.notify_one();
    }
  }
  // body(i0, i1) over nt contiguous parts of [0, n_); 1 <= nt_ <= workers + 1
  void parallel_for(int n_, int nt_, const std::function<void(int, int)>& body) {
    {
      std::lock_guard<std::mutex> l(m);
      fn = body;
      n = n_;
      nt = nt_;
      left = nt_ - 1;
      gen++;
    }
    go.notify_all();
    body(0, (int)((int64_t)n_ / nt_));
    std::unique_lock<std::mutex> l(m);
    done.wait(l, [&] { return left == 0; });
  }
};

}  // namespace sdsj
