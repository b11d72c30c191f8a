// Host AddressSanitizer / UBSan driver of the shared GIF core (sds_amd/csrc/sdsj_gif.h: the functions
// sdsj_gif_probe, host planning, k_parse, k_gif_lzw and k_gif_rgb run).  A plain serial decoder built from
// those functions -- parse, descriptor, LZW over the sub-block chain, index lookup, RGB -- reads records
// [u32 length][bytes] from the file in argv[1] and prints one line per record:
// status width height fnv1a64(RGB).  Each input, each index buffer and each RGB buffer is an exactly sized
// heap block, so any access past an end is reported.
#include "png_driver_common.h"

#include "../../sds_amd/csrc/sdsj_gif.h"

static int decode(const uint8_t* buf, int64_t n, GifHdr* h, unsigned long long* hash) {
  Rd rd{buf};
  int st = gif_parse(rd, n, h);
  if (st != SDSJ_OK) return st;
  ImgDesc* d = new ImgDesc();
  gif_fill_desc(d, *h);  // (the kernels read the frame back from the descriptor: so does this decoder)
  const GifView v = gif_view(*d);
  const int64_t expect = (int64_t)v.fw * v.fh;
  uint8_t* idx = static_cast<uint8_t*>(malloc((size_t)expect));
  GifTable* T = new GifTable();
  GifBits<Rd> br;
  gif_bits_init(br, rd, n, d->png_idat_pos);
  SerialSink sink{idx, 0};
  st = gif_lzw(br, T, sink, expect, d->png_depth_lace & 255);
  delete T;
  if (st == SDSJ_OK && sink.pos != expect) st = SDSJ_CORRUPT;
  if (st == SDSJ_OK) {
    const int w = d->width, ht = d->height;
    uint8_t* rgb = static_cast<uint8_t*>(malloc((size_t)w * ht * 3));
    // (a grey file has no table: an exactly sized empty block, never read)
    uint8_t* tab = static_cast<uint8_t*>(malloc(v.table_n ? (size_t)v.table_n * 3 : 1));
    if (v.table_n) memcpy(tab, buf + d->png_plte_pos, (size_t)v.table_n * 3);
    const Rd pal{tab}, ix{idx};
    for (int y = 0; y < ht; y++)
      for (int x = 0; x < w; x++) {
        const uint32_t c = gif_rgb(gif_index_at(v, ix, x, y), v.table_n, pal);
        uint8_t* o = rgb + ((int64_t)y * w + x) * 3;
        o[0] = (uint8_t)c;
        o[1] = (uint8_t)(c >> 8);
        o[2] = (uint8_t)(c >> 16);
      }
    *hash = fnv1a64(rgb, (int64_t)w * ht * 3);
    free(rgb);
    free(tab);
  }
  free(idx);
  delete d;
  return st;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  return for_each_record(argv[1], [](const uint8_t* buf, int64_t n) {
    GifHdr h;
    unsigned long long hash = 0;
    const int st = decode(buf, n, &h, &hash);
    printf("%d %d %d %llu\n", st, h.width, h.height, hash);
  });
}
