// What the host sanitizer drivers of the shared PNG core (png_driver.cpp, png_ext_driver.cpp,
// png_meta_driver.cpp) share: the byte reader, the serial inflate sink, inflate + Adler-32, the hash of the
// RGB and the loop over the input records.  Each driver keeps its own decode / status function and main.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../sds_amd/csrc/sdsj_png.h"

using namespace sdsj;

struct Rd {
  const uint8_t* p;
  int operator()(int64_t i) const { return p[i]; }
};

// The serial sink: what the device's WaveSink does with 64 lanes.
struct SerialSink {
  uint8_t* out;
  int64_t pos;
  void lit(int b) { out[pos++] = (uint8_t)b; }
  void match(int dist, int len) {
    for (int i = 0; i < len; i++) out[pos + i] = out[pos - dist + (i % dist)];
    pos += len;
  }
};

// png_inflate over the IDAT chain at idat_pos into raw[0, expect), then the serial Adler-32 against the stream's.
inline int inflate_checked(Rd rd, int64_t n, int64_t idat_pos, uint8_t* raw, int64_t expect) {
  InfTables* T = new InfTables();
  PngBits<Rd> br;
  png_bits_init(br, rd, n, idat_pos);
  SerialSink sink{raw, 0};
  uint32_t want = 0;
  int st = png_inflate(br, T, sink, expect, &want);
  delete T;
  if (st == SDSJ_OK) {
    uint32_t s1 = 1, s2 = 0;
    for (int64_t i = 0; i < expect; i++) {
      s1 = (s1 + raw[i]) % kAdlerMod;
      s2 = (s2 + s1) % kAdlerMod;
    }
    if (((s2 << 16) | s1) != want) st = SDSJ_CORRUPT;
  }
  return st;
}

inline unsigned long long fnv1a64(const uint8_t* p, int64_t n) {
  unsigned long long f = 1469598103934665603ull;
  for (int64_t i = 0; i < n; i++) f = (f ^ p[i]) * 1099511628211ull;
  return f;
}

// Calls fn(buf, n) for every record [u32 length][bytes] of the file, buf being an exactly sized heap block (one
// byte for an empty record), so any access past its end is reported.  Returns main's exit status.
template <class Fn>
int for_each_record(const char* path, Fn fn) {
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  std::vector<uint8_t> all;
  static uint8_t tmp[1 << 16];
  size_t r;
  while ((r = fread(tmp, 1, sizeof(tmp), f)) > 0) all.insert(all.end(), tmp, tmp + r);
  fclose(f);
  size_t pos = 0;
  while (pos + 4 <= all.size()) {
    uint32_t n;
    memcpy(&n, &all[pos], 4);
    pos += 4;
    if (pos + n > all.size()) return 3;
    uint8_t* buf = static_cast<uint8_t*>(malloc(n ? n : 1));
    memcpy(buf, &all[pos], n);
    pos += n;
    fn(buf, (int64_t)n);
    free(buf);
  }
  return 0;
}
