// Host AddressSanitizer / UBSan driver of the shared PNG core (sds_amd/csrc/sdsj_png.h: the functions
// sdsj_png_probe, host planning, k_parse, k_png_inflate and k_png_unfilter run).  A plain serial decoder
// built from those functions -- parse, inflate over the IDAT chain, Adler-32, filter bytes, unfilter,
// RGB -- reads records [u32 length][bytes] from the file in argv[1] and prints one line per record:
// status width height fnv1a64(RGB).  Each input, each scanline buffer and each RGB buffer is an
// exactly sized heap block, so any access past an end is reported.
#include "png_driver_common.h"

static int decode(const uint8_t* buf, int64_t n, PngHdr* h, unsigned long long* hash) {
  Rd rd{buf};
  int st = png_parse(rd, n, h);
  if (st != SDSJ_OK) return st;
  const int64_t expect = png_raw_bytes(h->width, h->height, h->bpp);
  uint8_t* raw = static_cast<uint8_t*>(malloc((size_t)expect));
  st = inflate_checked(rd, n, h->idat_pos, raw, expect);
  const int64_t pitch = 1 + (int64_t)h->width * h->bpp;
  for (int y = 0; st == SDSJ_OK && y < h->height; y++)
    if (raw[y * pitch] > 4) st = SDSJ_CORRUPT;
  if (st == SDSJ_OK) {
    const int w = h->width, bpp = h->bpp;
    uint8_t* rgb = static_cast<uint8_t*>(malloc((size_t)w * h->height * 3));
    std::vector<uint32_t> prev((size_t)w, 0u), cur((size_t)w, 0u);
    Rd pal{buf + h->plte_pos};
    for (int y = 0; y < h->height; y++) {
      const uint8_t* row = raw + y * pitch;
      for (int x = 0; x < w; x++) {
        uint32_t px = 0;
        for (int k = 0; k < bpp; k++) px |= (uint32_t)row[1 + (int64_t)x * bpp + k] << (8 * k);
        cur[x] = png_recon(row[0], px, x ? cur[x - 1] : 0u, prev[x], x ? prev[x - 1] : 0u, bpp);
        const uint32_t c = png_rgb(h->ctype, cur[x], h->plte_n, pal);
        uint8_t* o = rgb + ((int64_t)y * w + x) * 3;
        o[0] = (uint8_t)c;
        o[1] = (uint8_t)(c >> 8);
        o[2] = (uint8_t)(c >> 16);
      }
      prev.swap(cur);
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
