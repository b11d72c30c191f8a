// Host AddressSanitizer / UBSan driver of the shared TIFF core (sds_amd/csrc/sdsj_tiff.h: the functions
// sdsj_tiff_probe, host planning, k_parse, k_tiff_copy, k_tiff_lzw, k_tiff_inflate and k_tiff_rgb run).  A plain
// serial decoder built from those functions -- parse, descriptor, strip ranges, PackBits / LZW / Deflate per strip,
// predictor, RGB -- reads records [u32 length][bytes] from the file in argv[1] and prints one line per record:
// status width height fnv1a64(RGB).  Each input, each strip's output, the ColorMap and each RGB buffer is an
// exactly sized heap block, so any access past an end is reported.
#include "png_driver_common.h"

#include "../../sds_amd/csrc/sdsj_tiff.h"

// The serial PackBits sink: what the device's WaveRunSink does with 64 lanes.
struct SerialRunSink {
  uint8_t* out;
  const uint8_t* in;
  int64_t pos;
  void copy(int64_t src, int k) {
    for (int i = 0; i < k; i++) out[pos + i] = in[src + i];
    pos += k;
  }
  void fill(int b, int k) {
    for (int i = 0; i < k; i++) out[pos + i] = (uint8_t)b;
    pos += k;
  }
};

static int decode_strip(const uint8_t* buf, int64_t n, const TiffView& v, const TiffStrip& sp, uint8_t* out) {
  const Rd rd{buf};
  if (v.codec == kTiffNone) {
    memcpy(out, buf + sp.pos, (size_t)sp.expect);
    return SDSJ_OK;
  }
  if (v.codec == kTiffPackBits) {
    SerialRunSink sink{out, buf, 0};
    const int st = tiff_packbits(rd, sp.pos, sp.pos + sp.len, sink, sp.expect);
    return st == SDSJ_OK && sink.pos != sp.expect ? SDSJ_CORRUPT : st;
  }
  if (v.codec == kTiffLzw) {
    GifTable* T = new GifTable();
    TiffBits<Rd> br;
    tiff_bits_init(br, rd, sp.pos, sp.pos + sp.len);
    SerialSink sink{out, 0};
    int st = tiff_lzw(br, T, sink, sp.expect);
    delete T;
    return st == SDSJ_OK && sink.pos != sp.expect ? SDSJ_CORRUPT : st;
  }
  InfTables* T = new InfTables();
  PngBits<Rd> br;
  png_bits_span(br, rd, n, sp.pos, sp.pos + sp.len);
  SerialSink sink{out, 0};
  uint32_t want = 0;
  int st = tiff_inflate(br, T, sink, sp.expect, &want);
  delete T;
  if (st == SDSJ_OK) {
    uint32_t s1 = 1, s2 = 0;
    for (int64_t i = 0; i < sp.expect; i++) {
      s1 = (s1 + out[i]) % kAdlerMod;
      s2 = (s2 + s1) % kAdlerMod;
    }
    if (((s2 << 16) | s1) != want) st = SDSJ_CORRUPT;
  }
  return st;
}

static int decode(const uint8_t* buf, int64_t n, TiffHdr* h, unsigned long long* hash) {
  Rd rd{buf};
  int st = tiff_parse(rd, n, h);
  if (st != SDSJ_OK) return st;
  ImgDesc* d = new ImgDesc();
  tiff_fill_desc(d, *h);  // (the kernels read the layout back from the descriptor: so does this decoder)
  const TiffView v = tiff_view(*d);
  const int w = d->width, ht = d->height;
  uint8_t* rgb = static_cast<uint8_t*>(malloc((size_t)w * ht * 3));
  uint8_t* cm = static_cast<uint8_t*>(malloc(v.photo == 3 ? 1536 : 1));
  if (v.photo == 3) memcpy(cm, buf + v.cmap_pos, 1536);
  const Rd cmap{cm};
  for (int s = 0; s < v.nstrips && st == SDSJ_OK; s++) {
    TiffStrip sp;
    if (!tiff_strip(rd, n, v, w, ht, s, &sp) || (int64_t)sp.row0 * w * v.spp + sp.expect > d->png_raw) {
      st = SDSJ_CORRUPT;
      break;
    }
    uint8_t* out = static_cast<uint8_t*>(malloc((size_t)sp.expect));
    st = decode_strip(buf, n, v, sp, out);
    for (int r = 0; r < sp.rows && st == SDSJ_OK; r++) {
      const uint8_t* row = out + (int64_t)r * w * v.spp;
      uint32_t left = 0;
      for (int x = 0; x < w; x++) {
        uint32_t px = 0;
        for (int c = 0; c < v.spp; c++) px |= (uint32_t)row[(int64_t)x * v.spp + c] << (8 * c);
        if (v.predictor == 2) left = px = tiff_unpredict(px, left);
        const uint32_t c = tiff_rgb(px, v.photo, v.be, cmap);
        uint8_t* o = rgb + ((int64_t)(sp.row0 + r) * w + x) * 3;
        o[0] = (uint8_t)c;
        o[1] = (uint8_t)(c >> 8);
        o[2] = (uint8_t)(c >> 16);
      }
    }
    free(out);
  }
  if (st == SDSJ_OK) *hash = fnv1a64(rgb, (int64_t)w * ht * 3);
  free(cm);
  free(rgb);
  delete d;
  return st;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  return for_each_record(argv[1], [](const uint8_t* buf, int64_t n) {
    TiffHdr h;
    unsigned long long hash = 0;
    const int st = decode(buf, n, &h, &hash);
    printf("%d %d %d %llu\n", st, h.width, h.height, hash);
  });
}
