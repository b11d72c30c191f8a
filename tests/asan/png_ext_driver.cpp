// Host AddressSanitizer / UBSan driver of the shared PNG core under the full format mask
// (SDSJ_FORMAT_PNG | SDSJ_FORMAT_PNG_EXT): the functions k_parse, k_png_inflate and k_png_unfilter_ext
// run for Adam7 files and bit depths 1, 2, 4, 16 -- png_parse with the mask, png_layout, the 64-bit
// png_recon, png_rgb_ext.  A plain serial decoder like tests/asan/png_driver.cpp: it reads records
// [u32 length][bytes] from the file in argv[1] and prints one line per record: status width height
// fnv1a64(RGB).  Each input, each scanline buffer and each RGB buffer is an exactly sized heap block.
#include "png_driver_common.h"

static int decode(const uint8_t* buf, int64_t n, PngHdr* h, unsigned long long* hash) {
  Rd rd{buf};
  int st = png_parse(rd, n, h, SDSJ_FORMAT_JPEG | SDSJ_FORMAT_PNG | SDSJ_FORMAT_PNG_EXT);
  if (st != SDSJ_OK) return st;
  PngLayout L;
  png_layout(h->width, h->height, h->ctype, h->bit_depth, h->interlace, &L);
  if (L.unit != h->bpp) abort();  // (png_parse's filter unit is the layout's)
  const int64_t expect = L.total;
  uint8_t* raw = static_cast<uint8_t*>(malloc((size_t)expect));
  st = inflate_checked(rd, n, h->idat_pos, raw, expect);
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
    *hash = fnv1a64(rgb, (int64_t)w * h->height * 3);
    free(rgb);
  }
  free(raw);
  return st;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  return for_each_record(argv[1], [](const uint8_t* buf, int64_t n) {
    PngHdr h;
    unsigned long long hash = 0;
    const int st = decode(buf, n, &h, &hash);
    printf("%d %d %d %llu\n", st, h.width, h.height, hash);
  });
}
