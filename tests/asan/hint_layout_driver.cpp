// Host AddressSanitizer / UBSan driver of the subsequence layout by subsequence (sds_amd/csrc/sdsj_common.h:
// sub_count, sub_total, sub_interval, sub_layout) and of hint_entry_safe -- what k_enthint counts with and what
// a lane of k_entwrite builds for itself on a hinted image.  For seeded random interval tables it compares the
// per-lane functions, for every subsequence, with a plain serial restatement of ent_layout
// (sds_amd/csrc/sdsj_entropy.hip), and the count; then it runs the safety predicate at its edges.  Every table
// lives in exactly sized heap arrays, so a read past an end is reported.  Prints "ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../sds_amd/csrc/sdsj_common.h"

using namespace sdsj;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("line %d: %s (table %d)\n", __LINE__, #c, g_table);  \
      exit(1);                                                    \
    }                                                             \
  } while (0)

static int g_table = 0;
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull) >> 32);
}

struct Ref {
  uint32_t start_bit, end_bit, lim_bit;
  int32_t first, seg;
};

// ent_layout, one thread after another: interval s -> max(1, ceil(bits / SB)) subsequences in interval order,
// none at or past cap; returns their number
static int serial_layout(int nseg, const int32_t* lo, const int32_t* hi, uint32_t SB, int cap, std::vector<Ref>& out) {
  out.assign((size_t)(cap > 0 ? cap : 0), Ref{});
  int64_t carry = 0;
  for (int s = 0; s < nseg; s++) {
    const uint32_t b0 = (uint32_t)lo[s] * 8u;
    uint32_t b1 = (uint32_t)hi[s] * 8u;
    if (b1 < b0) b1 = b0;
    const int cnt = b1 > b0 ? (int)((b1 - b0 + SB - 1) / SB) : 1;
    for (int k = 0; k < cnt; k++) {
      const int64_t j = carry + k;
      if (j >= cap) break;
      Ref& S = out[(size_t)j];
      S.start_bit = b0 + (uint32_t)k * SB;
      const uint32_t e = S.start_bit + SB;
      S.end_bit = e < b1 ? e : b1;
      S.first = k == 0;
      S.seg = s;
      S.lim_bit = b1;
    }
    carry += cnt;
  }
  return carry < cap ? (int)carry : cap;
}

// a byte length whose bit count is `res` modulo SB (the smallest at or after `from`; none: `from`)
static int32_t len_with_residue(uint32_t SB, uint32_t res, int32_t from) {
  for (int32_t n = from; n < from + (int32_t)SB + 8; n++)
    if (((uint32_t)n * 8u) % SB == res) return n;
  return from;
}

static void one_table(int nseg, uint32_t SB, int cap_mode) {
  g_table++;
  // exactly sized arrays (lo and hi hold nseg + 1 entries on the device; the layout reads nseg of each)
  int32_t* lo = static_cast<int32_t*>(malloc(sizeof(int32_t) * (size_t)nseg));
  int32_t* hi = static_cast<int32_t*>(malloc(sizeof(int32_t) * (size_t)nseg));
  int32_t* off = static_cast<int32_t*>(malloc(sizeof(int32_t) * (size_t)nseg));
  int32_t pos = 8 + (int32_t)(rnd() % 64);  // (byte offsets are never negative: hi < lo stays above 0)
  for (int s = 0; s < nseg; s++) {
    const int32_t from = (int32_t)(rnd() % (3 * SB / 8 + 2));
    int32_t len;
    switch (rnd() % 7) {
      case 0: len = 0; break;                                     // an empty interval
      case 1: len = -(int32_t)(rnd() % 3); break;                 // hi <= lo
      case 2: len = len_with_residue(SB, SB - 1, from); break;    // 1 bit short of a multiple (where bytes allow)
      case 3: len = len_with_residue(SB, 0, from + 1); break;     // exactly a multiple
      case 4: len = len_with_residue(SB, 1 % SB, from); break;    // 1 bit over
      case 5: len = 1; break;
      default: len = from; break;
    }
    lo[s] = pos;
    hi[s] = pos + len;
    pos += (len > 0 ? len : 0) + (int32_t)(rnd() % 3);
  }
  int64_t sum = 0;
  for (int s = 0; s < nseg; s++) {  // the exclusive sums the device takes with a scan
    off[s] = (int32_t)sum;
    sum += sub_count(lo[s], hi[s], SB);
  }
  const int natural = (int)sum;
  int cap = natural;
  if (cap_mode == 0) cap = natural > 3 ? natural - 3 : 1;
  if (cap_mode == 1) cap = natural > 1 ? natural - 1 : 1;
  if (cap_mode == 3) cap = natural + 5;
  std::vector<Ref> ref;
  const int want = serial_layout(nseg, lo, hi, SB, cap, ref);
  const int got = sub_total(sum, cap);
  CHECK(got == want);
  for (int j = 0; j < got; j++) {
    const int s = sub_interval(off, nseg, j);
    CHECK(s >= 0 && s < nseg && off[s] <= j);
    const SubLayout o = sub_layout(lo[s], hi[s], SB, s, j - off[s], j, got);
    const Ref& R = ref[(size_t)j];
    CHECK(o.seg == R.seg);
    CHECK(o.first == (R.first != 0));
    CHECK(o.start_bit == R.start_bit);
    CHECK(o.end_bit == R.end_bit);
    CHECK(o.lim_bit == R.lim_bit);
    const bool last = j + 1 == got || ref[(size_t)j + 1].first != 0;  // as the write pass reads it from the SubStates
    CHECK(o.last == last);
  }
  free(lo);
  free(hi);
  free(off);
}

static void predicate_edges() {
  g_table = -1;
  SubLayout o{};
  o.start_bit = 4096;
  o.end_bit = 5120;
  o.lim_bit = 9000;
  o.seg = 2;
  o.first = false;
  o.last = false;
  const int bpm = 6;
  auto y = [](uint32_t blk, uint32_t nblk) { return (blk << 24) | nblk; };
  CHECK(!hint_entry_safe(o.start_bit - 1, y(0, 7), o, bpm));
  CHECK(hint_entry_safe(o.start_bit, y(0, 7), o, bpm));
  CHECK(hint_entry_safe(o.lim_bit + 2048, y(0, 7), o, bpm));
  CHECK(!hint_entry_safe(o.lim_bit + 2049, y(0, 7), o, bpm));
  CHECK(hint_entry_safe(o.start_bit, y(bpm - 1, 0xFFFFFF), o, bpm));
  CHECK(!hint_entry_safe(o.start_bit, y(bpm, 0), o, bpm));
  CHECK(!hint_entry_safe(o.start_bit, y(255, 0), o, bpm));
  // grayscale: block 0 only
  CHECK(hint_entry_safe(o.start_bit, y(0, 1), o, 1));
  CHECK(!hint_entry_safe(o.start_bit, y(1, 1), o, 1));
  // the bound does not wrap at 2^32
  o.start_bit = 0xFFFFF000u;
  o.lim_bit = 0xFFFFFFF0u;
  CHECK(hint_entry_safe(0xFFFFFFFFu, y(0, 0), o, bpm));
  CHECK(!hint_entry_safe(100u, y(0, 0), o, bpm));
  // an interval's first subsequence takes nothing from the record
  o.first = true;
  CHECK(hint_entry_safe(0u, y(255, 0), o, bpm));
}

int main() {
  const int nsegs[] = {1, 2, 3, 63, 64, 65, 255, 256};
  const uint32_t sbs[] = {1024, 1023, 1025, 777, 8};
  for (int nseg : nsegs)
    for (uint32_t SB : sbs)
      for (int cap_mode = 0; cap_mode < 4; cap_mode++)
        for (int rep = 0; rep < 6; rep++) one_table(nseg, SB, cap_mode);
  predicate_edges();
  printf("ok\n");
  return 0;
}
