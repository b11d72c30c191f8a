// Host AddressSanitizer / UBSan driver of the shared WebP core (sds_amd/csrc/sdsj_webp.h: the functions
// sdsj_webp_probe, host planning, k_parse, k_webp_decode, k_webp_inverse and k_webp_rgb run).  A plain serial
// decoder built from those functions -- container, descriptor, prefix codes, LZ77 with the colour cache, the
// inverse transforms, RGB -- reads records [u32 length][bytes] from the file in argv[1] and prints one line per
// record: status width height fnv1a64(RGB) groups.  Each input, each scratch block and each RGB buffer is an
// exactly sized heap block, so any access past an end is reported.  The last column is the number of prefix-code
// groups of the main image (the measurement behind kWebpMaxGroups).
#include "png_driver_common.h"

#include "../../sds_amd/csrc/sdsj_webp.h"

// The serial sink: what the device's WaveSink32 does with 64 lanes.
struct SerialSink32 {
  uint32_t* out;
  int64_t pos;
  uint32_t* cache;
  int cache_bits;
  int groups;
  void put(uint32_t v) {
    if (cache_bits) cache[(0x1E35A7BDu * v) >> (32 - cache_bits)] = v;
  }
  void begin(uint32_t* dst, int bits) {
    out = dst;
    pos = 0;
    cache_bits = bits;
    for (int i = 0; i < (bits ? 1 << bits : 0); i++) cache[i] = 0;
  }
  void lit(uint32_t v) {
    put(v);
    out[pos++] = v;
  }
  void cached(int key) { lit(cache[key]); }
  void match(int dist, int len) {
    for (int i = 0; i < len; i++) {
      out[pos] = out[pos - dist];
      put(out[pos++]);
    }
  }
  void finish() {}
  void load_codes(WebpCode* dst, const WebpCode* src) {
    for (int j = 0; j < 5; j++) dst[j] = src[j];
  }
  int max_group(const uint32_t* p, int64_t n) {
    uint32_t m = 0;
    for (int64_t i = 0; i < n; i++) m = ((p[i] >> 8) & 0xFFFFu) > m ? (p[i] >> 8) & 0xFFFFu : m;
    groups = (int)m + 1;
    return (int)m;
  }
};

static int decode(const uint8_t* buf, int64_t n, WebpHdr* h, unsigned long long* hash, int* groups) {
  Rd rd{buf};
  int st = webp_parse(rd, n, h);
  if (st != SDSJ_OK) return st;
  ImgDesc* d = new ImgDesc();
  webp_fill_desc(d, *h);  // (the kernels read the payload back from the descriptor: so does this decoder)
  const WebpView v = webp_view(*d);
  const int w = d->width, ht = d->height;
  const WebpLayout L = webp_layout(w, ht);
  uint8_t* mem = static_cast<uint8_t*>(malloc((size_t)d->png_raw));
  uint32_t* cache = static_cast<uint32_t*>(malloc(sizeof(uint32_t) << kWebpMaxCacheBits));
  WebpTmp* T = new WebpTmp();
  SerialSink32 sink{nullptr, 0, cache, 0, 1};
  st = d->png_raw == L.total ? webp_decode(rd, v, w, ht, mem, T, sink) : SDSJ_CORRUPT;
  *groups = sink.groups;
  delete T;
  free(cache);
  if (st == SDSJ_OK) {
    webp_inverse_serial(mem, w, ht, ht);
    const uint32_t* a = reinterpret_cast<const uint32_t*>(mem + L.argb);
    uint8_t* rgb = static_cast<uint8_t*>(malloc((size_t)w * ht * 3));
    for (int64_t p = 0; p < (int64_t)w * ht; p++) {
      rgb[3 * p] = (uint8_t)(a[p] >> 16);
      rgb[3 * p + 1] = (uint8_t)(a[p] >> 8);
      rgb[3 * p + 2] = (uint8_t)a[p];
    }
    *hash = fnv1a64(rgb, (int64_t)w * ht * 3);
    free(rgb);
  }
  free(mem);
  delete d;
  return st;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  return for_each_record(argv[1], [](const uint8_t* buf, int64_t n) {
    WebpHdr h;
    unsigned long long hash = 0;
    int groups = 0;
    const int st = decode(buf, n, &h, &hash, &groups);
    printf("%d %d %d %llu %d\n", st, h.width, h.height, hash, groups);
  });
}
