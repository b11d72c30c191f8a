// Host AddressSanitizer / UBSan driver of the shared PNG core under the full format mask
// (SDSJ_FORMAT_PNG | SDSJ_FORMAT_PNG_EXT): the functions k_parse, k_png_inflate and k_png_unfilter_ext
// run for Adam7 files and bit depths 1, 2, 4, 16 -- png_parse with the mask, png_layout, the 64-bit
// png_recon, png_rgb_ext.  A plain serial decoder like tests/asan/png_driver.cpp: it reads records
// [u32 length][bytes] from the file in argv[1] and prints one line per record: status width height
// fnv1a64(RGB).  Each input, each scanline buffer and each RGB buffer is an exactly sized heap block.
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

struct SerialSink {
  uint8_t* out;
  int64_t pos;
  void lit(int b) { out[pos++] = (uint8_t)b; }
  void match(int dist, int len) {
    for (int i = 0; i < len; i++) out[pos + i] = out[pos - dist + (i % dist)];
    pos += len;
  }
};

static int decode(const uint8_t* buf, int64_t n, PngHdr* h, unsigned long long* hash) {
  Rd rd{buf};
  int st = png_parse(rd, n, h, SDSJ_FORMAT_JPEG | SDSJ_FORMAT_PNG | SDSJ_FORMAT_PNG_EXT);
  if (st != SDSJ_OK) return st;
  PngLayout L;
  png_layout(h->width, h->height, h->ctype, h->bit_depth, h->interlace, &L);
  if (L.unit != h->bpp) abort();  // (png_parse's filter unit is the layout's)
  const int64_t expect = L.total;
  uint8_t* raw = static_cast<uint8_t*>(malloc((size_t)expect));
  InfTables* T = new InfTables();
  PngBits<Rd> br;
  png_bits_init(br, rd, n, h->idat_pos);
  SerialSink sink{raw, 0};
  uint32_t want = 0;
  st = png_inflate(br, T, sink, expect, &want);
  delete T;
  if (st == SDSJ_OK) {
    uint32_t s1 = 1, s2 = 0;
    for (int64_t i = 0; i < expect; i++) {
      s1 = (s1 + raw[i]) % kAdlerMod;
      s2 = (s2 + s1) % kAdlerMod;
    }
    if (((s2 << 16) | s1) != want) st = SDSJ_CORRUPT;
  }
  for (int p = 0; st == SDSJ_OK && p < L.npass; p++)
    for (int y = 0; y < L.pass[p].h; y++)
      if (raw[L.pass[p].off + y * (1 + L.pass[p].rowbytes)] > 4) st = SDSJ_CORRUPT;
  if (st == SDSJ_OK) {
    const int w = h->width, unit = L.unit, depth = h->bit_depth;
    const int ppu = depth < 8 ? 8 / depth : 1;
    uint8_t* rgb = static_cast<uint8_t*>(malloc((size_t)w * h->height * 3));
    Rd pal{buf + h->plte_pos};
    for (int p = 0; p < L.npass; p++) {
      const PngPass& ps = L.pass[p];
      const int nu = (int)(ps.rowbytes / unit);
      std::vector<uint64_t> prev((size_t)nu, 0u), cur((size_t)nu, 0u);
      for (int py = 0; py < ps.h; py++) {
        const uint8_t* row = raw + ps.off + py * (1 + ps.rowbytes);
        for (int u = 0; u < nu; u++) {
          uint64_t px = 0;
          for (int k = 0; k < unit; k++) px |= (uint64_t)row[1 + (int64_t)u * unit + k] << (8 * k);
          cur[u] = png_recon(row[0], px, u ? cur[u - 1] : (uint64_t)0, prev[u], u ? prev[u - 1] : (uint64_t)0, unit);
          for (int k = 0; k < ppu; k++) {
            const int pxl = u * ppu + k;
            if (pxl >= ps.w) break;
            const uint32_t c = png_rgb_ext(h->ctype, depth, cur[u], k, h->plte_n, pal);
            uint8_t* o = rgb + ((int64_t)(ps.ys + py * ps.dy) * w + (ps.xs + pxl * ps.dx)) * 3;
            o[0] = (uint8_t)c;
            o[1] = (uint8_t)(c >> 8);
            o[2] = (uint8_t)(c >> 16);
          }
        }
        prev.swap(cur);
      }
    }
    unsigned long long f = 1469598103934665603ull;
    for (int64_t i = 0; i < (int64_t)w * h->height * 3; i++) f = (f ^ rgb[i]) * 1099511628211ull;
    *hash = f;
    free(rgb);
  }
  free(raw);
  return st;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
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
    PngHdr h;
    unsigned long long hash = 0;
    const int st = decode(buf, (int64_t)n, &h, &hash);
    printf("%d %d %d %llu\n", st, h.width, h.height, hash);
    free(buf);
  }
  return 0;
}
