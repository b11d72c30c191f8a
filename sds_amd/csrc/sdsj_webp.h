// sdsj_webp.h -- the WebP subset the MI355X path decodes (SDSJ_FORMAT_WEBP): the RIFF container and the
// whole lossless codec (VP8L, RFC 9649), as functions shared by the host (sdsj_webp_probe, host planning, the
// serial decoder of tests/asan/webp_driver.cpp) and the device (k_parse, k_webp_decode, k_webp_inverse,
// k_webp_rgb in sdsj_webp.hip).  Every decision about correctness or bounds is taken here; the kernels add
// only the lane-parallel movement of pixels.
//
// Reference behaviour: PIL.Image.open(...).convert("RGB") (WebPImagePlugin.py over libwebp 1.6.0's
// WebPAnimDecoder, Pillow 12.2.0): the coded pixels, alpha dropped without compositing.
//   - RIFF + size + WEBP, then a VP8L chunk, or VP8X (10 bytes, no flag outside alpha / animation / EXIF /
//     ICCP / XMP) followed by chunks, of which ICCP, EXIF, "XMP " and unknown ones are skipped; the canvas
//     must equal the VP8L frame; one image chunk only.  Animation (flag, ANIM, ANMF) and lossy files
//     ("VP8 ", ALPH) are SDSJ_UNSUPPORTED.  Chunks are padded to even sizes, bytes after the RIFF size are
//     ignored, a RIFF or chunk size past the input is SDSJ_CORRUPT
//   - VP8L: signature 0x2F, 14 + 14 bits of size minus one, the alpha bit (no part in convert("RGB")),
//     version 0; up to four transforms, each type once (predictor and cross-colour with a sub-image at
//     size_bits 2..9, subtract-green, colour-indexing with a delta-coded table of 1..256 entries and 8 / 4 /
//     2 / 1 pixels per word, an index at or beyond the table giving 0x00000000); an optional colour cache of
//     1..11 bits; on the main image an optional meta-prefix image (prefix_bits 2..9); five prefix codes per
//     group (simple or normal; a code of one symbol reads no bits; every other code must be complete, as
//     libwebp's VP8LBuildHuffmanTable demands); LZ77 with the 120 short distance codes
//   - predictor modes 0..13 with libwebp's border rules; modes 14 and 15 predict 0xFF000000 like mode 0
//     (found from a synthesised file against PIL)
//   - reading a bit beyond the chunk's last byte fails, wherever it happens (libwebp's sticky end-of-stream)
// The rule is exactness, as for PNG and GIF: SDSJ_OK only where PIL decodes the same bytes to the same
// pixels without raising; a valid file outside the subset is SDSJ_UNSUPPORTED, anything malformed or unsure
// SDSJ_CORRUPT, and the transforms rerun both on PIL, which then decides.
#pragma once
#include <stdint.h>

#include "sdsj_common.h"
#include "sdsj_gif.h"  // kGifMaxHeader
#include "sdsj_png.h"  // SDSJ_HDI, kPngMaxPixels

namespace sdsj {

constexpr int kWebpSample = 3;        // ImgDesc::png of a WebP sample
constexpr int kWebpMaxGroups = 256;   // prefix-code groups of the main image this path keeps tables for ("WebP")
constexpr int kWebpMaxCacheBits = 11;
constexpr int kWebpGreen = 256 + 24 + (1 << kWebpMaxCacheBits);  // the largest alphabet
constexpr int kWebpLutBits = 8;

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDSJ_HDN __host__ __device__ __attribute__((noinline))
#else
#define SDSJ_HDN __attribute__((noinline))
#endif

struct WebpHdr {
  int32_t width, height, has_alpha, lossless, extended;
  int64_t data_pos, data_end;  // the VP8L chunk's payload
};

template <class Reader>
SDSJ_HD inline bool webp_signature(const Reader& rd, int64_t n) {
  return n >= 12 && rd(0) == 'R' && rd(1) == 'I' && rd(2) == 'F' && rd(3) == 'F' && rd(8) == 'W' && rd(9) == 'E' &&
         rd(10) == 'B' && rd(11) == 'P';
}

template <class Reader>
SDSJ_HDI uint32_t webp_le32(const Reader& rd, int64_t i) {
  return (uint32_t)rd(i) | ((uint32_t)rd(i + 1) << 8) | ((uint32_t)rd(i + 2) << 16) | ((uint32_t)rd(i + 3) << 24);
}
template <class Reader>
SDSJ_HDI bool webp_tag(const Reader& rd, int64_t i, char a, char b, char c, char d) {
  return rd(i) == a && rd(i + 1) == b && rd(i + 2) == c && rd(i + 3) == d;
}

// The five header bytes of a VP8L payload at p (inside the input).
template <class Reader>
SDSJ_HDI int webp_vp8l_header(const Reader& rd, int64_t p, int64_t end, WebpHdr* h) {
  if (end - p < 5) return SDSJ_CORRUPT;
  if (rd(p) != 0x2F) return SDSJ_CORRUPT;
  const uint32_t v = webp_le32(rd, p + 1);
  h->width = (int32_t)(v & 0x3FFFu) + 1;
  h->height = (int32_t)((v >> 14) & 0x3FFFu) + 1;
  h->has_alpha = (int32_t)((v >> 28) & 1u);
  if (v >> 29) return SDSJ_UNSUPPORTED;  // a version this path does not know (libwebp refuses it)
  return SDSJ_OK;
}

// The size of a lossy key frame ("VP8 " payload at p): for sdsj_webp_probe only.
template <class Reader>
SDSJ_HDI void webp_vp8_size(const Reader& rd, int64_t p, int64_t end, WebpHdr* h) {
  if (end - p < 10 || (rd(p) & 1) || rd(p + 3) != 0x9D || rd(p + 4) != 0x01 || rd(p + 5) != 0x2A) return;
  h->width = (rd(p + 6) | (rd(p + 7) << 8)) & 0x3FFF;
  h->height = (rd(p + 8) | (rd(p + 9) << 8)) & 0x3FFF;
}

// Container and VP8L header: everything knowable without reading prefix-coded data.  h's size is filled as
// soon as it has been read, whatever the status.  No byte outside [0, n) is read; the walk is bounded by the
// input's length (a chunk takes at least eight bytes).
// (Inlined into k_parse like gif_parse: kept out of line it cost k_parse 10% under the default mask, a call in the
// kernel giving it a stack; inlined it costs 2.5%.)
template <class Reader>
SDSJ_HD int webp_parse(const Reader& rd, int64_t n, WebpHdr* h) {
  h->width = h->height = h->has_alpha = h->extended = 0;
  h->lossless = 0;
  h->data_pos = h->data_end = 0;
  if (!webp_signature(rd, n)) return SDSJ_UNSUPPORTED;
  const int64_t riff = (int64_t)webp_le32(rd, 4);
  if (n < 20) return SDSJ_CORRUPT;
  if (riff < 12 || (riff & 1) || riff + 8 > n) return SDSJ_CORRUPT;
  const int64_t end = riff + 8;  // (bytes after it are ignored)
  int64_t p = 12;
  int cw = 0, ch = 0, seen = 0, st = SDSJ_OK;
  if (webp_tag(rd, p, 'V', 'P', '8', 'X')) {
    if (webp_le32(rd, p + 4) != 10u || end < 30) return SDSJ_CORRUPT;
    const int flags = rd(p + 8);
    cw = (rd(p + 12) | (rd(p + 13) << 8) | (rd(p + 14) << 16)) + 1;
    ch = (rd(p + 15) | (rd(p + 16) << 8) | (rd(p + 17) << 16)) + 1;
    h->extended = 1;
    h->width = cw <= 0x4000 ? cw : 0;  // (a VP8L frame has at most 14 bits of size)
    h->height = ch <= 0x4000 ? ch : 0;
    h->has_alpha = (flags >> 4) & 1;
    if (flags & ~0x3E) return SDSJ_CORRUPT;
    if (flags & 2) return SDSJ_UNSUPPORTED;  // animation
    if (rd(p + 9) | rd(p + 10) | rd(p + 11)) return SDSJ_CORRUPT;  // (reserved: unsure)
    p = 30;
  }
  for (;;) {
    if (p == end && seen) break;
    if (end - p < 8) return SDSJ_CORRUPT;
    if (!seen && p > kGifMaxHeader) return SDSJ_UNSUPPORTED;
    const int64_t size = (int64_t)webp_le32(rd, p + 4), padded = size + (size & 1);
    if (padded > end - p - 8) return SDSJ_CORRUPT;
    const int64_t q = p + 8;
    if (webp_tag(rd, p, 'V', 'P', '8', 'L')) {
      if (seen) return SDSJ_CORRUPT;
      seen = 1;
      h->lossless = 1;
      const int has_alpha = h->has_alpha;
      st = webp_vp8l_header(rd, q, q + size, h);
      if (h->extended) h->has_alpha = has_alpha | h->has_alpha;
      if (st == SDSJ_CORRUPT) return st;
      h->data_pos = q;
      h->data_end = q + size;
      if (!h->extended) break;  // (a bare file: nothing after the image is looked at)
    } else if (webp_tag(rd, p, 'V', 'P', '8', ' ') || webp_tag(rd, p, 'A', 'L', 'P', 'H')) {
      if (!seen && rd(p + 3) == ' ') webp_vp8_size(rd, q, q + size, h);
      return seen ? SDSJ_CORRUPT : SDSJ_UNSUPPORTED;  // lossy
    } else if (webp_tag(rd, p, 'A', 'N', 'I', 'M') || webp_tag(rd, p, 'A', 'N', 'M', 'F')) {
      return seen ? SDSJ_CORRUPT : SDSJ_UNSUPPORTED;
    } else if (webp_tag(rd, p, 'V', 'P', '8', 'X') || !h->extended) {
      return SDSJ_CORRUPT;  // (a bare file starts with its image chunk)
    }
    p = q + padded;
  }
  if (st != SDSJ_OK) return st;
  if (h->extended && (h->width != cw || h->height != ch)) return SDSJ_UNSUPPORTED;  // canvas and frame differ
  if ((int64_t)h->width * h->height > kPngMaxPixels) return SDSJ_UNSUPPORTED;
  return SDSJ_OK;
}

// ------------------------------------------------------------------------------------------
// The scratch of one sample, known from width and height alone (an upper bound: the transform headers sit
// behind prefix-coded data).  Offsets in bytes from the sample's off_png, each a multiple of 256.
// ------------------------------------------------------------------------------------------
struct WebpCode {
  uint16_t lut[1 << kWebpLutBits];  // by the next 8 bits: length << 12 | symbol; 0: a longer code
  uint16_t count[16];               // codes per length; count[0] == 0xFFFF: a code of one symbol (count[1]), no bits
};
struct WebpGroup {
  WebpCode c[5];  // green + length + cache, red, blue, alpha, distance
  uint16_t sorted[kWebpGreen + 3 * 256 + 40];  // the symbols of each code by (length, symbol)
};
SDSJ_HDI int webp_alphabet(int j, int cache_bits) {
  return j == 0 ? 256 + 24 + (cache_bits > 0 ? 1 << cache_bits : 0) : j == 4 ? 40 : 256;
}
SDSJ_HDI int webp_sorted_at(int j) { return j == 0 ? 0 : j == 4 ? kWebpGreen + 3 * 256 : kWebpGreen + (j - 1) * 256; }

struct WebpState {  // what k_webp_decode leaves for k_webp_inverse and k_webp_rgb, at the start of the scratch
  int32_t ntrans;
  int32_t type[4], bits[4], xsize[4];  // in reading order; xsize: the width the transform's output has
  int32_t coded_xsize;                 // the width of the coded main image
  int32_t ctab_n;
};
struct WebpLayout {
  int64_t state, argb, sub[3], ctab, groups, total;  // sub: meta-prefix, predictor, cross-colour; groups: [0] serves the sub-images
};
SDSJ_HD inline int64_t webp_sub_words(int w, int h) { return (int64_t)((w + 3) >> 2) * ((h + 3) >> 2); }
SDSJ_HD inline WebpLayout webp_layout(int w, int h) {
  WebpLayout l;
  int64_t o = 0;
  l.state = o;
  o += 256;
  l.argb = o;
  o += align_up((int64_t)w * h * 4, 256);
  for (int i = 0; i < 3; i++) {
    l.sub[i] = o;
    o += align_up(webp_sub_words(w, h) * 4, 256);
  }
  l.ctab = o;  // 256 entries as the inverse pass reads them, then the up to 256 delta-coded words as decoded
  o += 2048;
  l.groups = o;
  o += align_up((int64_t)(kWebpMaxGroups + 1) * (int64_t)sizeof(WebpGroup), 256);
  l.total = o;
  return l;
}

// What the kernels need of a WebP descriptor (webp_fill_desc packs it into the PNG fields).
struct WebpView {
  int64_t data_pos, data_end;
};
SDSJ_HD inline WebpView webp_view(const ImgDesc& d) { return WebpView{d.png_idat_pos, d.png_plte_pos}; }

// The descriptor of a parsed WebP: like a PNG's and a GIF's it has no components, blocks or entropy data,
// and neither the PNG nor the GIF kernels meet it (its route is kRtWebp; they test png == 1 / 2).
SDSJ_HD inline void webp_fill_desc(ImgDesc* d, const WebpHdr& h) {
  d->width = h.width;
  d->height = h.height;
  d->ncomp = 0;
  d->hmax = d->vmax = 1;
  d->mcux = d->mcuy = d->bpm = 0;
  d->restart_interval = 0;
  d->nseg = 1;
  d->saw_jfif = d->saw_adobe = d->adobe_transform = 0;
  d->entropy_off = d->entropy_len = 0;
  d->total_blocks = 0;
  d->progressive = 0;
  d->sos_pos = 0;
  d->png = kWebpSample;
  d->png_ctype = h.has_alpha;
  d->png_bpp = 4;
  d->png_plte_n = 0;
  d->png_plte_pos = h.data_end;
  d->png_idat_pos = h.data_pos;
  d->png_raw = h.width > 0 && h.height > 0 ? webp_layout(h.width, h.height).total : 0;
  d->png_depth_lace = 8;
  d->off_png = 0;
}

// ------------------------------------------------------------------------------------------
// Bit reader over the payload [pos, end), LSB first.  Beyond the end it reads zero bits and sets `eos` once a
// bit past the last byte has been consumed; every caller fails on it.  No byte outside [pos, end) is read.
// ------------------------------------------------------------------------------------------
template <class Reader>
struct WebpBits {
  Reader rd;
  int64_t pos, end;
  uint64_t buf;
  int32_t cnt, eos;
};
template <class Reader>
SDSJ_HDI void webp_bits_init(WebpBits<Reader>& b, const Reader& rd, int64_t pos, int64_t end) {
  b.rd = rd;
  b.pos = pos;
  b.end = end;
  b.buf = 0;
  b.cnt = 0;
  b.eos = 0;
}
template <class Reader>
SDSJ_HDI void webp_fill(WebpBits<Reader>& b) {  // at least 32 bits: the longest read
  if (b.cnt >= 32) return;
  while (b.cnt <= 56) {
    const uint64_t v = b.pos < b.end ? (uint64_t)(uint32_t)b.rd(b.pos) : 0ull;
    b.buf |= v << b.cnt;
    b.pos++;  // (past the end it counts the zero bytes handed out)
    b.cnt += 8;
  }
}
template <class Reader>
SDSJ_HDI void webp_drop(WebpBits<Reader>& b, int k) {
  b.buf >>= k;
  b.cnt -= k;
  if ((b.pos - b.end) * 8 > (int64_t)b.cnt) b.eos = 1;
}
template <class Reader>
SDSJ_HDI uint32_t webp_take(WebpBits<Reader>& b, int k) {  // k <= 32
  if (k == 0) return 0;
  webp_fill(b);
  const uint32_t v = (uint32_t)(b.buf & ((1ull << k) - 1));
  webp_drop(b, k);
  return v;
}

// A prefix code from its lengths cl[0, n): false where libwebp's VP8LBuildHuffmanTable returns 0 (no
// symbol, a length above 15, an incomplete or over-subscribed code) and for the one case this path is not
// sure about (one symbol of length 15).  One pass counts, one places the symbols and fills the table.
SDSJ_HDN inline bool webp_build(const uint8_t* cl, int n, WebpCode* c, uint16_t* sorted) {
  int count[16], next[16], off[16];
  for (int i = 0; i < 16; i++) count[i] = 0;
  int last = 0;
  for (int s = 0; s < n; s++) {
    if (cl[s] > 15) return false;
    count[cl[s]]++;
    if (cl[s]) last = s;
  }
  const int used = n - count[0];
  if (used == 0) return false;
  if (used == 1) {
    if (cl[last] == 15) return false;
    c->count[0] = 0xFFFF;
    c->count[1] = (uint16_t)last;
    sorted[0] = (uint16_t)last;
    return true;
  }
  int64_t left = 1;
  for (int len = 1; len <= 15; len++) {
    left = (left << 1) - count[len];
    if (left < 0) return false;
  }
  if (left != 0) return false;
  int code = 0, o = 0;
  c->count[0] = 0;
  for (int len = 1; len <= 15; len++) {
    c->count[len] = (uint16_t)count[len];
    next[len] = code;
    off[len] = o;
    o += count[len];
    code = (code + count[len]) << 1;
  }
  for (int s = 0; s < n; s++) {
    const int len = cl[s];
    if (!len) continue;
    sorted[off[len]++] = (uint16_t)s;
    const int k = next[len]++;
    if (len <= kWebpLutBits) {
      int rev = 0;
      for (int i = 0; i < len; i++) rev |= ((k >> i) & 1) << (len - 1 - i);
      for (int i = rev; i < (1 << kWebpLutBits); i += 1 << len) c->lut[i] = (uint16_t)((len << 12) | s);
    } else {
      const int top = k >> (len - kWebpLutBits);
      int rev = 0;
      for (int i = 0; i < kWebpLutBits; i++) rev |= ((top >> i) & 1) << (kWebpLutBits - 1 - i);
      c->lut[rev] = 0;
    }
  }
  return true;
}

template <class Reader>
SDSJ_HDI int webp_symbol(WebpBits<Reader>& b, const WebpCode* c, const uint16_t* sorted) {
  if (c->count[0] == 0xFFFF) return c->count[1];
  webp_fill(b);
  const uint32_t e = c->lut[b.buf & ((1u << kWebpLutBits) - 1)];
  if (e >> 12) {
    webp_drop(b, (int)(e >> 12));
    return (int)(e & 0xFFFu);
  }
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= 15; len++) {
    code |= (int)((b.buf >> (len - 1)) & 1u);
    const int cnt = c->count[len];
    if (code - cnt < first) {
      webp_drop(b, len);
      return sorted[index + (code - first)];
    }
    index += cnt;
    first = (first + cnt) << 1;
    code <<= 1;
  }
  b.eos = 1;  // (cannot happen: the code is complete)
  return 0;
}

// The memory a decode works in besides the scratch: the lengths being read and the code-length code.
struct WebpTmp {
  uint8_t cl[kWebpGreen];
  WebpCode clc;
  uint16_t cls[19];
  WebpCode cur[5];  // the tables of the group being decoded (webp_pixels), next to the reader: LDS on the device
};

// One prefix code of an alphabet of n symbols (ReadHuffmanCode).
template <class Reader>
SDSJ_HDI int webp_read_code_impl(WebpBits<Reader>& b, WebpTmp* T, int n, WebpCode* c, uint16_t* sorted) {
  for (int i = 0; i < n; i++) T->cl[i] = 0;
  if (webp_take(b, 1)) {  // simple
    const int two = (int)webp_take(b, 1);
    const int s0 = (int)webp_take(b, webp_take(b, 1) ? 8 : 1);
    if (s0 < n) T->cl[s0] = 1;
    if (two) {
      const int s1 = (int)webp_take(b, 8);
      if (s1 < n) T->cl[s1] = 1;
    }
  } else {
    const uint8_t order[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    uint8_t ccl[19];
    for (int i = 0; i < 19; i++) ccl[i] = 0;
    const int num = (int)webp_take(b, 4) + 4;
    for (int i = 0; i < num; i++) ccl[order[i]] = (uint8_t)webp_take(b, 3);
    if (!webp_build(ccl, 19, &T->clc, T->cls)) return SDSJ_CORRUPT;
    int max_symbol = n;
    if (webp_take(b, 1)) {
      const int nb = 2 + 2 * (int)webp_take(b, 3);
      max_symbol = 2 + (int)webp_take(b, nb);
      if (max_symbol > n) return SDSJ_CORRUPT;
    }
    int s = 0, prev = 8;
    while (s < n) {
      if (max_symbol-- == 0) break;
      const int v = webp_symbol(b, &T->clc, T->cls);
      if (b.eos) return SDSJ_CORRUPT;
      if (v < 16) {
        T->cl[s++] = (uint8_t)v;
        if (v) prev = v;
      } else {
        const int extra = v == 16 ? 2 : v == 17 ? 3 : 7;
        const int rep = (int)webp_take(b, extra) + (v == 18 ? 11 : 3);
        if (s + rep > n) return SDSJ_CORRUPT;
        const int fill = v == 16 ? prev : 0;
        for (int i = 0; i < rep; i++) T->cl[s++] = (uint8_t)fill;
      }
    }
  }
  if (b.eos) return SDSJ_CORRUPT;
  return webp_build(T->cl, n, c, sorted) ? SDSJ_OK : SDSJ_CORRUPT;
}

// (Not inlined, to keep the kernel small; the reader's state is copied to a local for the call, so that it
// lives in registers and not behind the caller's reference.)
template <class Reader>
SDSJ_HDN int webp_read_code(WebpBits<Reader>& b, WebpTmp* T, int n, WebpCode* c, uint16_t* sorted) {
  WebpBits<Reader> lb = b;
  const int st = webp_read_code_impl(lb, T, n, c, sorted);
  b = lb;
  return st;
}

template <class Reader>
SDSJ_HDI int webp_read_group(WebpBits<Reader>& b, WebpTmp* T, WebpGroup* g, int cache_bits) {
  for (int j = 0; j < 5; j++) {
    const int st = webp_read_code(b, T, webp_alphabet(j, cache_bits), &g->c[j], g->sorted + webp_sorted_at(j));
    if (st != SDSJ_OK) return st;
  }
  return SDSJ_OK;
}

// The distance of a distance code in an image xsize wide (libwebp's PlaneCodeToDistance): codes 1..120 name
// a neighbour (dx, dy), kept here as dy << 4 | 8 - dx; a distance below 1 is 1.
SDSJ_HDN inline int64_t webp_plane_distance(int xsize, int64_t code) {
  const uint8_t map[120] = {
      0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a,
      0x25, 0x2b, 0x48, 0x04, 0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03,
      0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d, 0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e,
      0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e, 0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f,
      0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e, 0x00, 0x74, 0x7c, 0x41,
      0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70};
  if (code > 120) return code - 120;
  const int m = map[code - 1];
  const int64_t dist = (int64_t)(m >> 4) * xsize + (8 - (m & 15));
  return dist < 1 ? 1 : dist;
}

// The value of a length or distance prefix symbol with its extra bits (GetCopyDistance).
template <class Reader>
SDSJ_HDI int64_t webp_prefix_value(WebpBits<Reader>& b, int sym) {
  if (sym < 4) return sym + 1;
  const int extra = (sym - 2) >> 1;
  const int64_t offset = (int64_t)(2 + (sym & 1)) << extra;
  return offset + (int64_t)webp_take(b, extra) + 1;
}

// The pixels of one entropy-coded image, xsize x ysize, into the sink (DecodeImageData):
//   out.lit(argb)         appends a pixel (and puts it into the colour cache)
//   out.cached(key)       appends the colour cache's entry
//   out.match(dist, len)  appends len pixels copied from dist pixels back (overlap allowed), caching each
//   out.load_codes(d, s)  copies a group's five WebpCode from the scratch to T->cur
// The sink never sees a pixel beyond xsize * ysize or a source before the first pixel.  `meta` (null: one
// group) is the meta-prefix image.  The loop ends after xsize * ysize pixels; a code of one symbol reads no
// bits, so it is the pixel count, not the input, that bounds it.
template <class Reader, class Sink>
SDSJ_HDI int webp_pixels_impl(WebpBits<Reader>& b, WebpTmp* T, const WebpGroup* groups, int ngroups, const uint32_t* meta,
                              int prefix_bits, int xsize, int ysize, int cache_bits, Sink& out) {
  const int64_t total = (int64_t)xsize * ysize;
  const int mask = meta ? (1 << prefix_bits) - 1 : -1;
  const int mxs = meta ? (xsize + mask) >> prefix_bits : 0;
  const int cache_limit = 280 + (cache_bits > 0 ? 1 << cache_bits : 0);
  int64_t done = 0;
  int x = 0, y = 0;
  const WebpGroup* g = groups;
  const WebpCode* c = T->cur;
  out.load_codes(T->cur, g->c);
  bool pick = true;
  while (done < total) {
    if (pick || (x & mask) == 0) {
      if (meta) {
        const int gi = (int)((meta[(int64_t)(y >> prefix_bits) * mxs + (x >> prefix_bits)] >> 8) & 0xFFFFu);
        if (gi >= ngroups) return SDSJ_CORRUPT;  // (cannot happen: ngroups is the image's maximum + 1)
        if (groups + gi != g) {
          g = groups + gi;
          out.load_codes(T->cur, g->c);
        }
      }
      pick = false;
    }
    const int code = webp_symbol(b, &c[0], g->sorted);
    if (code < 256) {
      const uint32_t red = (uint32_t)webp_symbol(b, &c[1], g->sorted + webp_sorted_at(1));
      const uint32_t blue = (uint32_t)webp_symbol(b, &c[2], g->sorted + webp_sorted_at(2));
      const uint32_t alpha = (uint32_t)webp_symbol(b, &c[3], g->sorted + webp_sorted_at(3));
      if (b.eos) return SDSJ_CORRUPT;
      out.lit((alpha << 24) | (red << 16) | ((uint32_t)code << 8) | blue);
      done++;
      if (++x >= xsize) {
        x = 0;
        y++;
      }
    } else if (code < 280) {
      const int64_t len = webp_prefix_value(b, code - 256);
      const int ds = webp_symbol(b, &c[4], g->sorted + webp_sorted_at(4));
      const int64_t dist = webp_plane_distance(xsize, webp_prefix_value(b, ds));
      if (b.eos) return SDSJ_CORRUPT;
      if (dist > done || len > total - done || dist > 0x7FFFFFFF) return SDSJ_CORRUPT;
      out.match((int)dist, (int)len);
      done += len;
      int64_t nx = x + len;
      y += (int)(nx / xsize);
      x = (int)(nx % xsize);
      pick = true;
    } else if (code < cache_limit) {
      out.cached(code - 280);
      done++;
      if (++x >= xsize) {
        x = 0;
        y++;
      }
    } else {
      return SDSJ_CORRUPT;
    }
  }
  return b.eos ? SDSJ_CORRUPT : SDSJ_OK;
}

// (Not inlined; reader and sink are copied to locals for the call, as in webp_read_code: the loop keeps their
// state in registers.)
template <class Reader, class Sink>
SDSJ_HDN int webp_pixels(WebpBits<Reader>& b, WebpTmp* T, const WebpGroup* groups, int ngroups, const uint32_t* meta,
                         int prefix_bits, int xsize, int ysize, int cache_bits, Sink& out) {
  WebpBits<Reader> lb = b;
  Sink lo = out;
  const int st = webp_pixels_impl(lb, T, groups, ngroups, meta, prefix_bits, xsize, ysize, cache_bits, lo);
  b = lb;
  out = lo;
  return st;
}

// The colour-cache bits in front of an image's codes: 0 none, -1 invalid.
template <class Reader>
SDSJ_HDI int webp_cache_bits(WebpBits<Reader>& b) {
  if (!webp_take(b, 1)) return 0;
  const int bits = (int)webp_take(b, 4);
  return bits >= 1 && bits <= kWebpMaxCacheBits ? bits : -1;
}

// A sub-image (predictor / cross-colour data, the meta-prefix image, the colour table): cache bits, one
// group of codes (built in *g), the pixels into dst through the sink.
template <class Reader, class Sink>
SDSJ_HDN int webp_sub_image(WebpBits<Reader>& b, WebpTmp* T, WebpGroup* g, Sink& out, uint32_t* dst, int xsize, int ysize) {
  const int cache_bits = webp_cache_bits(b);
  if (cache_bits < 0 || b.eos) return SDSJ_CORRUPT;
  int st = webp_read_group(b, T, g, cache_bits);
  if (st != SDSJ_OK) return st;
  out.begin(dst, cache_bits);
  st = webp_pixels(b, T, g, 1, nullptr, 0, xsize, ysize, cache_bits, out);
  out.finish();
  return st;
}

// The whole VP8L payload [v.data_pos, v.data_end) of a width x height image into the scratch at `mem` (laid
// out by webp_layout): the transforms' data, the state for the inverse passes, the coded ARGB image.
//   out.begin(dst, cache_bits)  starts an image at dst with an empty (zeroed) colour cache
//   out.finish()                completes its stores, so that they can be read back
//   out.max_group(p, n)         the largest group number (bits 8..23) among n words at p
// SDSJ_UNSUPPORTED: more groups than kWebpMaxGroups.
template <class Reader, class Sink>
SDSJ_HDI int webp_decode(const Reader& rd, const WebpView& v, int width, int height, uint8_t* mem, WebpTmp* T, Sink& out) {
  const WebpLayout L = webp_layout(width, height);
  WebpState* S = reinterpret_cast<WebpState*>(mem + L.state);
  WebpGroup* groups = reinterpret_cast<WebpGroup*>(mem + L.groups);
  uint32_t* ctab = reinterpret_cast<uint32_t*>(mem + L.ctab);
  WebpBits<Reader> b;
  webp_bits_init(b, rd, v.data_pos + 5, v.data_end);
  if (v.data_end - v.data_pos < 5) return SDSJ_CORRUPT;
  int xsize = width, ntrans = 0, seen = 0;
  S->ntrans = 0;
  S->ctab_n = 0;
  while (webp_take(b, 1)) {
    if (b.eos || ntrans == 4) return SDSJ_CORRUPT;
    const int type = (int)webp_take(b, 2);
    if ((seen >> type) & 1) return SDSJ_CORRUPT;
    seen |= 1 << type;
    S->type[ntrans] = type;
    S->xsize[ntrans] = xsize;
    S->bits[ntrans] = 0;
    if (type == 0 || type == 1) {
      const int bits = (int)webp_take(b, 3) + 2;
      S->bits[ntrans] = bits;
      const int sw = (xsize + (1 << bits) - 1) >> bits, sh = (height + (1 << bits) - 1) >> bits;
      if ((int64_t)sw * sh > webp_sub_words(width, height)) return SDSJ_CORRUPT;  // (cannot happen: bits >= 2)
      const int st = webp_sub_image(b, T, groups, out, reinterpret_cast<uint32_t*>(mem + L.sub[1 + type]), sw, sh);
      if (st != SDSJ_OK) return st;
    } else if (type == 3) {
      const int n = (int)webp_take(b, 8) + 1;
      const int bits = n > 16 ? 0 : n > 4 ? 1 : n > 2 ? 2 : 3;
      S->bits[ntrans] = bits;
      S->ctab_n = n;
      const uint32_t* raw = ctab + 256;  // (decoded next to the table, so that the sums below never overwrite a word still to be read)
      const int st = webp_sub_image(b, T, groups, out, ctab + 256, n, 1);
      if (st != SDSJ_OK) return st;
      // delta-coded; entries at and beyond n read as 0x00000000 (libwebp zero-fills the expanded map)
      uint32_t prev = 0;
      for (int i = 0; i < 256; i++) {
        const uint32_t c = i < n ? raw[i] : 0u;
        const uint32_t s = i < n ? (((c & 0xFF00FF00u) + (prev & 0xFF00FF00u)) & 0xFF00FF00u) | (((c & 0x00FF00FFu) + (prev & 0x00FF00FFu)) & 0x00FF00FFu) : 0u;
        ctab[i] = s;
        prev = s;
      }
      out.finish();
      xsize = (xsize + (1 << bits) - 1) >> bits;
    }
    ntrans++;
    S->ntrans = ntrans;
  }
  S->coded_xsize = xsize;
  if (b.eos) return SDSJ_CORRUPT;
  const int cache_bits = webp_cache_bits(b);
  if (cache_bits < 0 || b.eos) return SDSJ_CORRUPT;
  const uint32_t* meta = nullptr;
  int prefix_bits = 0, ngroups = 1;
  if (webp_take(b, 1)) {
    prefix_bits = (int)webp_take(b, 3) + 2;
    const int mw = (xsize + (1 << prefix_bits) - 1) >> prefix_bits, mh = (height + (1 << prefix_bits) - 1) >> prefix_bits;
    uint32_t* m = reinterpret_cast<uint32_t*>(mem + L.sub[0]);
    if ((int64_t)mw * mh > webp_sub_words(width, height)) return SDSJ_CORRUPT;
    const int st = webp_sub_image(b, T, groups, out, m, mw, mh);
    if (st != SDSJ_OK) return st;
    ngroups = out.max_group(m, (int64_t)mw * mh) + 1;
    meta = m;
  }
  if (b.eos) return SDSJ_CORRUPT;
  if (ngroups > kWebpMaxGroups) return SDSJ_UNSUPPORTED;
  for (int i = 0; i < ngroups; i++) {
    const int st = webp_read_group(b, T, groups + 1 + i, cache_bits);
    if (st != SDSJ_OK) return st;
  }
  out.begin(reinterpret_cast<uint32_t*>(mem + L.argb), cache_bits);
  const int st = webp_pixels(b, T, groups + 1, ngroups, meta, prefix_bits, xsize, height, cache_bits, out);
  out.finish();
  return st;
}

// ------------------------------------------------------------------------------------------
// Inverse transforms, per pixel.
// ------------------------------------------------------------------------------------------
SDSJ_HDI uint32_t webp_add(uint32_t a, uint32_t b) {  // per channel, modulo 256
  return (((a & 0xFF00FF00u) + (b & 0xFF00FF00u)) & 0xFF00FF00u) | (((a & 0x00FF00FFu) + (b & 0x00FF00FFu)) & 0x00FF00FFu);
}
SDSJ_HDI uint32_t webp_avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xFEFEFEFEu) >> 1) + (a & b); }
SDSJ_HDI int webp_clip255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
SDSJ_HDI int webp_abs(int v) { return v < 0 ? -v : v; }

// The predictor of `mode` (bits 8..11 of the predictor image's pixel) from the neighbours left, top,
// top-left and top-right.  Modes 14 and 15 predict like mode 0 (libwebp; found against PIL).
SDSJ_HDI uint32_t webp_predict(int mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
  switch (mode) {
    case 1: return L;
    case 2: return T;
    case 3: return TR;
    case 4: return TL;
    case 5: return webp_avg2(webp_avg2(L, TR), T);
    case 6: return webp_avg2(L, TL);
    case 7: return webp_avg2(L, T);
    case 8: return webp_avg2(TL, T);
    case 9: return webp_avg2(T, TR);
    case 10: return webp_avg2(webp_avg2(L, TL), webp_avg2(T, TR));
    case 11: {
      int d = 0;  // sum |L - TL| - sum |T - TL|: at or below zero T, else L
      for (int s = 0; s < 32; s += 8) {
        const int l = (int)((L >> s) & 255u), t = (int)((T >> s) & 255u), tl = (int)((TL >> s) & 255u);
        d += webp_abs(l - tl) - webp_abs(t - tl);
      }
      return d <= 0 ? T : L;
    }
    case 12: {
      uint32_t r = 0;
      for (int s = 0; s < 32; s += 8)
        r |= (uint32_t)webp_clip255((int)((L >> s) & 255u) + (int)((T >> s) & 255u) - (int)((TL >> s) & 255u)) << s;
      return r;
    }
    case 13: {
      const uint32_t a = webp_avg2(L, T);
      uint32_t r = 0;
      for (int s = 0; s < 32; s += 8) {
        const int x = (int)((a >> s) & 255u), y = (int)((TL >> s) & 255u);
        r |= (uint32_t)webp_clip255(x + (x - y) / 2) << s;
      }
      return r;
    }
    default: return 0xFF000000u;  // 0, 14, 15
  }
}
// The mode that holds at (x, y) whatever the predictor image says: libwebp's border rules.
SDSJ_HDI int webp_border_mode(int mode, int x, int y) { return y == 0 ? (x == 0 ? 0 : 1) : x == 0 ? 2 : mode; }

SDSJ_HDI uint32_t webp_add_green(uint32_t p) {
  const uint32_t g = (p >> 8) & 255u;
  return (p & 0xFF00FF00u) | (((p & 0x00FF00FFu) + ((g << 16) | g)) & 0x00FF00FFu);
}
SDSJ_HDI int webp_ctd(int t, int c) { return ((int)(int8_t)t * (int)(int8_t)c) >> 5; }
SDSJ_HDI uint32_t webp_cross(uint32_t code, uint32_t p) {  // code: red_to_blue << 16 | green_to_blue << 8 | green_to_red
  const int green = (int)((p >> 8) & 255u);
  int red = (int)((p >> 16) & 255u), blue = (int)(p & 255u);
  red = (red + webp_ctd((int)(code & 255u), green)) & 255;
  blue = (blue + webp_ctd((int)((code >> 8) & 255u), green)) & 255;
  blue = (blue + webp_ctd((int)((code >> 16) & 255u), red)) & 255;
  return (p & 0xFF00FF00u) | ((uint32_t)red << 16) | (uint32_t)blue;
}
// Pixel x of a row from its packed words (colour indexing with `bits`: 8 >> bits bits per pixel, in green).
SDSJ_HDI uint32_t webp_indexed(const uint32_t* ctab, uint32_t word, int x, int bits) {
  const int per = 8 >> bits;
  const uint32_t idx = (((word >> 8) & 255u) >> ((x & ((1 << bits) - 1)) * per)) & ((1u << per) - 1u);
  return ctab[idx];
}

// The inverse transforms over rows [0, rows) of the image at `mem`, serially, in place, in reverse order of
// reading: what k_webp_inverse does with 64 lanes.  The image's pitch is always `width` pixels.
SDSJ_HD inline void webp_inverse_serial(uint8_t* mem, int width, int height, int rows) {
  const WebpLayout L = webp_layout(width, height);
  const WebpState* S = reinterpret_cast<const WebpState*>(mem + L.state);
  uint32_t* a = reinterpret_cast<uint32_t*>(mem + L.argb);
  const uint32_t* ctab = reinterpret_cast<const uint32_t*>(mem + L.ctab);
  for (int i = S->ntrans - 1; i >= 0; i--) {
    const int xs = S->xsize[i], bits = S->bits[i];
    if (S->type[i] == 2) {
      for (int64_t p = 0; p < (int64_t)xs * rows; p++) a[p] = webp_add_green(a[p]);
    } else if (S->type[i] == 1) {
      const uint32_t* sub = reinterpret_cast<const uint32_t*>(mem + L.sub[2]);
      const int sw = (xs + (1 << bits) - 1) >> bits;
      for (int y = 0; y < rows; y++)
        for (int x = 0; x < xs; x++) a[(int64_t)y * xs + x] = webp_cross(sub[(int64_t)(y >> bits) * sw + (x >> bits)], a[(int64_t)y * xs + x]);
    } else if (S->type[i] == 3) {
      const int ps = (xs + (1 << bits) - 1) >> bits;
      for (int64_t p = (int64_t)xs * rows - 1; p >= 0; p--) {  // backwards: a word is read before its place is written
        const int y = (int)(p / xs), x = (int)(p % xs);
        a[p] = webp_indexed(ctab, a[(int64_t)y * ps + (x >> bits)], x, bits);
      }
    } else {
      const uint32_t* sub = reinterpret_cast<const uint32_t*>(mem + L.sub[1]);
      const int sw = (xs + (1 << bits) - 1) >> bits;
      for (int y = 0; y < rows; y++)
        for (int x = 0; x < xs; x++) {
          const int64_t p = (int64_t)y * xs + x;
          const int mode = webp_border_mode((int)((sub[(int64_t)(y >> bits) * sw + (x >> bits)] >> 8) & 15u), x, y);
          const uint32_t l = x ? a[p - 1] : 0u, t = y ? a[p - xs] : 0u, tl = x && y ? a[p - xs - 1] : 0u;
          const uint32_t tr = y ? a[p - xs + 1] : 0u;  // (past the row's end: the first pixel of this row)
          a[p] = webp_add(a[p], webp_predict(mode, l, t, tl, tr));
        }
    }
  }
}

}  // namespace sdsj
