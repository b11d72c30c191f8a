// Host ASan/UBSan driver for sds_amd/csrc/sdsj_buffers.h (tests/test_asan_buffers.py): Buf and Handle with
// a counting allocator that can fail its k-th allocation, and the staging layout.  Exits 0 and prints
// "ok" when every check holds; a failed check prints its line and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <utility>

#include "sdsj_buffers.h"

using namespace sdsj;

#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      printf("line %d: check failed: %s\n", __LINE__, #c);   \
      exit(1);                                               \
    }                                                        \
  } while (0)

namespace {

struct Counting {
  static int allocs, frees, calls, fail_at;  // fail_at: the 1-based allocation call that fails (0: none)
  static bool double_free;
  static std::set<void*> live;
  static void reset(int fail = 0) {
    CHECK(live.empty());
    allocs = frees = calls = 0;
    fail_at = fail;
  }
  static void* alloc(size_t bytes) {
    if (++calls == fail_at) return nullptr;
    void* p = malloc(bytes ? bytes : 1);
    live.insert(p);
    allocs++;
    return p;
  }
  static void free(void* p) {
    if (!live.erase(p)) {  // freed twice, or never allocated: recorded instead of handed to ::free
      double_free = true;
      return;
    }
    frees++;
    ::free(p);
  }
  static void balanced() {
    CHECK(!double_free);
    CHECK(live.empty());
    CHECK(frees == allocs);
  }
};
int Counting::allocs = 0, Counting::frees = 0, Counting::calls = 0, Counting::fail_at = 0;
bool Counting::double_free = false;
std::set<void*> Counting::live;

template <class T>
using B = Buf<T, Counting>;

void test_buf() {
  Counting::reset();
  {
    B<int64_t> a;
    CHECK(!a && a.get() == nullptr && a.size() == 0);
    CHECK(a.reserve(10) && a && a.size() == 10);
    for (int i = 0; i < 10; i++) a.get()[i] = i;  // (ASan: the allocation holds size() elements)
    int64_t* first = a.get();
    CHECK(a.reserve(1000) && a.size() == 1000);  // regrow: the old allocation is freed first
    CHECK(Counting::frees == 1 && !Counting::live.count(first));
    a.get()[999] = 1;
    B<int64_t> b(std::move(a));  // move-construct: the source is empty
    CHECK(!a && a.size() == 0 && b.size() == 1000 && b.get()[999] == 1);
    B<int64_t> c;
    CHECK(c.reserve(3));
    c = std::move(b);  // move-assign: c's allocation is freed, b is empty
    CHECK(!b && c.size() == 1000 && Counting::frees == 2);
    B<int64_t>& cr = c;
    c = std::move(cr);  // self-assign keeps the allocation
    CHECK(c.size() == 1000);
    c.reset();
    CHECK(!c && c.size() == 0 && Counting::frees == 3);
    c.reset();  // (an empty buffer frees nothing)
    CHECK(Counting::frees == 3);
    CHECK(c.reserve(5));
  }  // destructors: c's 5 elements only
  CHECK(Counting::allocs == 4);
  Counting::balanced();
}

struct Four {
  B<uint8_t> a;
  B<int32_t> b;
  B<int64_t> c;
  B<uint8_t> d;
  bool reserve_all(size_t n) { return a.reserve(n) && b.reserve(n) && c.reserve(n) && d.reserve(n); }
};

void test_failure_positions() {
  for (int round = 0; round < 2; round++)  // round 1: every buffer holds an earlier allocation when the failure comes
    for (int k = 1; k <= 4; k++) {
      Counting::reset();
      {
        Four f;
        if (round) CHECK(f.reserve_all(8));
        Counting::fail_at = Counting::calls + k;
        CHECK(!f.reserve_all(64));
        const bool empty[4] = {!f.a, !f.b, !f.c, !f.d};
        const size_t size[4] = {f.a.size(), f.b.size(), f.c.size(), f.d.size()};
        for (int j = 0; j < 4; j++) {
          if (j + 1 < k) CHECK(!empty[j] && size[j] == 64);     // allocated before the failure
          if (j + 1 == k) CHECK(empty[j] && size[j] == 0);      // the failed buffer is empty
          if (j + 1 > k) CHECK(size[j] == (round ? 8u : 0u));   // not reached: untouched
        }
        CHECK(f.reserve_all(16));  // and the struct is usable again
      }
      Counting::balanced();
      CHECK(Counting::allocs == (round ? 4 : 0) + (k - 1) + 4);
    }
}

struct IntDestroy {
  static int destroyed;
  static void destroy(int* p) {
    destroyed++;
    delete p;
  }
};
int IntDestroy::destroyed = 0;

void test_handle() {
  using H = Handle<int*, IntDestroy>;
  {
    H a;
    CHECK(!a && a.get() == nullptr);
    *a.put() = new int(1);
    CHECK(a && *a.get() == 1);
    H b(std::move(a));
    CHECK(!a && b && *b.get() == 1);
    H c;
    *c.put() = new int(2);
    c = std::move(b);  // destroys 2
    CHECK(IntDestroy::destroyed == 1 && !b && *c.get() == 1);
    *c.put() = new int(3);  // put on a full handle destroys 1 first
    CHECK(IntDestroy::destroyed == 2);
    H d;
  }  // destroys 3; the empty handles destroy nothing
  CHECK(IntDestroy::destroyed == 3);
}

void test_layout() {
  const int ms[] = {0, 1, 15, 16, 17, 4096};
  const int64_t totals[] = {0, 1, 16, 1 << 20};
  for (int m : ms)
    for (int64_t bytes : totals) {
      const StageLayout l = stage_layout(m, bytes);
      // the regions, in order: samples, offsets (int64), lengths (int32), flip bytes
      const int64_t begin[4] = {0, l.offsets, l.lengths, l.flip};
      const int64_t size[4] = {bytes, (int64_t)m * 8, (int64_t)m * 4, m};
      for (int r = 0; r < 4; r++) {
        CHECK(begin[r] % 16 == 0);
        const int64_t next = r < 3 ? begin[r + 1] : l.total;
        CHECK(begin[r] + size[r] <= next);  // in order and disjoint
        CHECK(next - (begin[r] + size[r]) < 16);  // (no more than the alignment between them)
      }
      CHECK(l.total % 16 == 0);
      CHECK(l.total == ((bytes + 15) / 16 + ((int64_t)m * 8 + 15) / 16 + ((int64_t)m * 4 + 15) / 16 + (m + 15) / 16) * 16);
    }
}

}  // namespace

int main() {
  test_buf();
  test_failure_positions();
  test_handle();
  test_layout();
  printf("ok\n");
  return 0;
}
