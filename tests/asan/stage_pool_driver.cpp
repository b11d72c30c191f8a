// Host ThreadSanitizer driver for sds_amd/csrc/sdsj_stage_pool.h (tests/test_asan_buffers.py): 200
// parallel_for calls of mixed n (some below the thread count) and mixed nt, each summing a known array
// into per-part slots, then the pool's destruction.  Exits 0 and prints "ok" when every sum is right.
#include <stdio.h>

#include <numeric>
#include <vector>

#include "sdsj_stage_pool.h"

int main() {
  const int workers = 7;
  std::vector<int64_t> data(5000);
  std::iota(data.begin(), data.end(), 1);
  int bad = 0;
  {
    sdsj::StagePool pool(workers);
    const int ns[] = {0, 1, 3, 7, 8, 33, 100, 1000, 4999, 5000};
    for (int call = 0; call < 200; call++) {
      const int n = ns[call % 10];
      const int nt = 1 + (call * 5 + call / 10) % (workers + 1);  // 1 .. workers + 1
      std::vector<int64_t> part(n + 1, 0);                        // (one slot per range start: no shared writes)
      std::vector<int> seen(n, 0);
      pool.parallel_for(n, nt, [&](int i0, int i1) {
        for (int i = i0; i < i1; i++) {
          part[i0] += data[i];
          seen[i]++;
        }
      });
      const int64_t sum = std::accumulate(part.begin(), part.end(), (int64_t)0);
      if (sum != (int64_t)n * (n + 1) / 2) bad++;
      for (int i = 0; i < n; i++)
        if (seen[i] != 1) bad++;  // every index exactly once
    }
  }  // joins the workers
  if (bad) {
    printf("%d wrong sums or indices\n", bad);
    return 1;
  }
  printf("ok\n");
  return 0;
}
