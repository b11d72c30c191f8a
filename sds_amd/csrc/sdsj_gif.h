// sdsj_gif.h -- the GIF subset the MI355X path decodes (SDSJ_FORMAT_GIF), as functions shared by the host
// (sdsj_gif_probe, host planning, the serial decoder of tests/asan/gif_driver.cpp) and the device (k_parse,
// k_gif_lzw, k_gif_rgb in sdsj_gif.hip).  Every decision about correctness or bounds is taken here; the
// kernels add only the lane-parallel movement of bytes.
//
// Reference behaviour: PIL.Image.open(...).convert("RGB") (GifImagePlugin.py + GifDecode.c, Pillow 12.2.0,
// LOADING_STRATEGY RGB_AFTER_FIRST): the first frame on the logical screen.
//   - GIF87a and GIF89a; the image has the logical screen's size (a frame that leaves the screen grows the
//     image there: SDSJ_UNSUPPORTED here)
//   - only the first image descriptor is decoded and nothing after its data is read
//   - a table that is the identity grey ramp (entry i = (i, i, i) for every entry: _is_palette_needed) counts
//     as no table; the colour table is the local one if there is one, else the global one; a pixel is
//     table[index], black at or beyond the table's entries; without either the image opens as mode L and a
//     pixel is (index, index, index) for every index.  A local grey ramp does not hide a global colour table:
//     _seek then sets mode L but copies the global palette, and Image.load puts it on the core image, which
//     turns to mode P -- convert("RGB") looks the indices up in the global table
//   - pixels outside the frame rectangle take the colour of index 0, or of the transparent index of a
//     graphic-control extension whose transparency flag is set; inside the frame that index is drawn like
//     any other; the screen's background byte plays no part
//   - interlaced frames: rows 0, 8, ..; 4, 12, ..; 2, 6, ..; 1, 3, ..
//   - LZW: codes LSB first, minimum code size + 1 up to 12 bits; clear and end codes; a full table takes no
//     more entries and stays at 12 bits until a clear; data after the last pixel is ignored, an end code is
//     not needed; an end code or the end of the sub-block chain before the last pixel raises OSError
// The rule is exactness, as for PNG: SDSJ_OK only where PIL decodes the same bytes to the same pixels
// without raising; a valid file outside the subset is SDSJ_UNSUPPORTED, anything malformed or unsure
// SDSJ_CORRUPT, and the transforms rerun both on PIL, which then decides.
#pragma once
#include <stdint.h>

#include "sdsj_common.h"
#include "sdsj_png.h"  // SDSJ_HDI, kPngMaxPixels

namespace sdsj {

constexpr int kGifSample = 2;             // ImgDesc::png of a GIF sample: non-zero ("no scan, unfused passes"), not 1
constexpr int64_t kGifMaxHeader = 1 << 20;  // bytes before the first image descriptor this path walks
constexpr int kGifTable = 4096;           // LZW codes (12 bits)

struct GifHdr {
  int32_t width, height;       // the logical screen
  int32_t fx, fy, fw, fh;      // the first frame's rectangle
  int32_t interlace;
  int32_t table_n;             // entries of the effective colour table; 0: grey (index, index, index)
  int32_t min_code;            // LZW minimum code size
  int32_t fill;                // index of the pixels outside the frame
  int64_t table_pos;           // first byte of the effective colour table
  int64_t data_pos;            // length byte of the first data sub-block
};

template <class Reader>
SDSJ_HD inline bool gif_signature(const Reader& rd, int64_t n) {
  return n >= 6 && rd(0) == 'G' && rd(1) == 'I' && rd(2) == 'F' && rd(3) == '8' && (rd(4) == '7' || rd(4) == '9') &&
         rd(5) == 'a';
}

template <class Reader>
SDSJ_HDI int gif_le16(const Reader& rd, int64_t i) {
  return rd(i) | (rd(i + 1) << 8);
}

// The identity grey ramp over `entries` entries at p (all inside the input): _is_palette_needed is false.
template <class Reader>
SDSJ_HDI bool gif_grey_ramp(const Reader& rd, int64_t p, int entries) {
  for (int i = 0; i < entries; i++)
    if (rd(p + 3 * i) != i || rd(p + 3 * i + 1) != i || rd(p + 3 * i + 2) != i) return false;
  return true;
}

// Signature, logical screen, global table, the blocks up to the first image descriptor, its local table
// and the minimum code size: up to the first data sub-block.  h's screen size is filled as soon as it has
// been read, whatever the status.  No byte outside [0, n) is read.
template <class Reader>
SDSJ_HD int gif_parse(const Reader& rd, int64_t n, GifHdr* h) {
  h->width = h->height = h->fx = h->fy = h->fw = h->fh = h->interlace = h->table_n = h->min_code = h->fill = 0;
  h->table_pos = h->data_pos = 0;
  if (!gif_signature(rd, n)) return SDSJ_UNSUPPORTED;
  if (n < 13) return SDSJ_CORRUPT;
  h->width = gif_le16(rd, 6);
  h->height = gif_le16(rd, 8);
  if (h->width == 0 || h->height == 0) return SDSJ_CORRUPT;
  if ((int64_t)h->width * h->height > kPngMaxPixels) return SDSJ_UNSUPPORTED;
  int64_t p = 13;
  int table_n = 0;  // entries of the effective table so far; -1: a grey ramp
  int64_t table_pos = 0;
  if (rd(10) & 128) {
    const int entries = 2 << (rd(10) & 7);
    if (p + 3 * entries > n) return SDSJ_CORRUPT;
    table_pos = p;
    table_n = gif_grey_ramp(rd, p, entries) ? -1 : entries;
    p += 3 * entries;
  }
  int fill = 0;
  for (;;) {
    if (p > kGifMaxHeader) return SDSJ_UNSUPPORTED;
    if (p >= n) return SDSJ_UNSUPPORTED;  // no image descriptor before the end of the input
    const int intro = rd(p++);
    if (intro == ';') return SDSJ_UNSUPPORTED;  // the trailer: no image
    if (intro == ',') break;
    if (intro != '!') return SDSJ_UNSUPPORTED;  // an unknown block introducer
    if (p >= n) return SDSJ_CORRUPT;
    const int label = rd(p++);
    // graphic control (249), comment (254), application (255), plain text (1): walked by their sub-blocks
    if (label != 249 && label != 254 && label != 255 && label != 1) return SDSJ_UNSUPPORTED;
    bool first = true;
    for (;;) {
      if (p >= n) return SDSJ_CORRUPT;
      const int len = rd(p++);
      if (len == 0) break;
      if (p + len > n) return SDSJ_CORRUPT;  // a sub-block that runs past the input
      if (first && label == 249) {
        if (len != 4) return SDSJ_UNSUPPORTED;  // (PIL indexes the block's fourth byte)
        if (rd(p) & 1) fill = rd(p + 3);
      }
      first = false;
      p += len;
      if (p > kGifMaxHeader) return SDSJ_UNSUPPORTED;
    }
  }
  if (p + 9 > n) return SDSJ_CORRUPT;
  h->fx = gif_le16(rd, p);
  h->fy = gif_le16(rd, p + 2);
  h->fw = gif_le16(rd, p + 4);
  h->fh = gif_le16(rd, p + 6);
  const int flags = rd(p + 8);
  p += 9;
  h->interlace = (flags >> 6) & 1;
  if (flags & 128) {
    const int entries = 2 << (flags & 7);
    if (p + 3 * entries > n) return SDSJ_CORRUPT;
    if (!gif_grey_ramp(rd, p, entries)) {  // (a local ramp leaves the global table in force)
      table_pos = p;
      table_n = entries;
    }
    p += 3 * entries;
  }
  if (p >= n) return SDSJ_CORRUPT;
  h->min_code = rd(p++);
  h->data_pos = p;
  h->table_n = table_n > 0 ? table_n : 0;
  h->table_pos = table_n > 0 ? table_pos : 0;
  h->fill = fill;
  if (h->fw == 0 || h->fh == 0) return SDSJ_CORRUPT;
  if (h->fx + h->fw > h->width || h->fy + h->fh > h->height) return SDSJ_UNSUPPORTED;  // PIL grows the image
  if (h->min_code < 2 || h->min_code > 8) return SDSJ_UNSUPPORTED;
  return SDSJ_OK;
}

// Row r of the frame (0 .. fh - 1) as a row of the LZW stream: itself, or its place in the four passes.
SDSJ_HD inline int gif_stream_row(int r, int fh, int interlace) {
  if (!interlace) return r;
  const int n1 = (fh + 7) >> 3, n2 = (fh + 3) >> 3, n3 = (fh + 1) >> 2;
  if ((r & 7) == 0) return r >> 3;
  if ((r & 7) == 4) return n1 + (r >> 3);
  if ((r & 3) == 2) return n1 + n2 + (r >> 2);
  return n1 + n2 + n3 + (r >> 1);
}

// What k_gif_rgb needs of a GIF descriptor (gif_fill_desc packs it into the PNG fields).
struct GifView {
  int fx, fy, fw, fh, interlace, fill, table_n;
};
SDSJ_HD inline GifView gif_view(const ImgDesc& d) {
  const uint32_t xy = (uint32_t)d.png_ctype, wh = (uint32_t)d.png_bpp, dl = (uint32_t)d.png_depth_lace;
  return GifView{(int)(xy & 0xFFFFu), (int)(xy >> 16), (int)(wh & 0xFFFFu), (int)(wh >> 16), (int)((dl >> 8) & 1u),
                 (int)((dl >> 16) & 255u), d.png_plte_n};
}

// Index of the screen's pixel (x, y): the frame's pixel from the LZW stream `idx` (fw x fh bytes in stream
// order), the fill index outside the frame.
template <class Idx>
SDSJ_HD inline int gif_index_at(const GifView& v, const Idx& idx, int x, int y) {
  const int fx = x - v.fx, fy = y - v.fy;
  if (fx < 0 || fy < 0 || fx >= v.fw || fy >= v.fh) return v.fill;
  return idx((int64_t)gif_stream_row(fy, v.fh, v.interlace) * v.fw + fx);
}

// The pixel of an index as convert("RGB") gives it: r | g << 8 | b << 16.  `pal(i)` returns table byte i.
template <class Pal>
SDSJ_HD inline uint32_t gif_rgb(int index, int table_n, const Pal& pal) {
  const uint32_t v = (uint32_t)index & 255u;
  if (table_n == 0) return v | (v << 8) | (v << 16);
  if ((int)v >= table_n) return 0;
  return (uint32_t)pal(3 * (int)v) | ((uint32_t)pal(3 * (int)v + 1) << 8) | ((uint32_t)pal(3 * (int)v + 2) << 16);
}

// The descriptor of a parsed GIF: like a PNG's it has no components, blocks or entropy data (every JPEG
// kernel tests `png`), and the PNG kernels never meet it (its route is kRtGif, and they test png == 1).
// ImgDesc keeps its size and offsets: the PNG fields carry what the GIF kernels need.
SDSJ_HD inline void gif_fill_desc(ImgDesc* d, const GifHdr& h) {
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
  d->png = kGifSample;
  d->png_ctype = (int32_t)((uint32_t)h.fx | ((uint32_t)h.fy << 16));
  d->png_bpp = (int32_t)((uint32_t)h.fw | ((uint32_t)h.fh << 16));
  d->png_plte_n = h.table_n;
  d->png_plte_pos = h.table_pos;
  d->png_idat_pos = h.data_pos;
  d->png_raw = (int64_t)h.width * h.height;  // the LZW stream takes the frame's fw x fh bytes of it
  d->png_depth_lace = (h.min_code & 255) | ((h.interlace & 1) << 8) | ((h.fill & 255) << 16);
  d->off_png = 0;
}

// ------------------------------------------------------------------------------------------
// Bit reader over the data sub-blocks (LSB first).  A sub-block is a length byte and that many data bytes;
// length 0 ends the chain, and so does the end of the input.  A sub-block that runs past the input sets
// `overrun` and ends the data.  No byte outside [0, n) is read.
// ------------------------------------------------------------------------------------------
template <class Reader>
struct GifBits {
  Reader rd;  // (by value: a reader with state, such as the device's LDS window, keeps it in registers)
  int64_t n, pos, blk_end;
  uint64_t buf;
  int32_t cnt;
  int32_t ended, overrun;
};

template <class Reader>
SDSJ_HDI void gif_bits_init(GifBits<Reader>& b, const Reader& rd, int64_t n, int64_t data_pos) {
  b.rd = rd;
  b.n = n;
  b.pos = b.blk_end = data_pos;
  b.buf = 0;
  b.cnt = 0;
  b.ended = b.overrun = 0;
}

template <class Reader>
SDSJ_HDI bool gif_hop(GifBits<Reader>& b) {  // positions on the next data byte; false: none
  while (b.pos == b.blk_end) {
    if (b.ended) return false;
    if (b.blk_end >= b.n) {
      b.ended = 1;
      return false;
    }
    const int len = b.rd(b.blk_end);
    if (len == 0) {
      b.ended = 1;
      return false;
    }
    if (b.blk_end + 1 + len > b.n) {
      b.ended = b.overrun = 1;
      return false;
    }
    b.pos = b.blk_end + 1;
    b.blk_end = b.pos + len;
  }
  return true;
}

template <class Reader>
SDSJ_HDI bool gif_take(GifBits<Reader>& b, int k, uint32_t* v) {  // k <= 12 bits; false: data exhausted
  while (b.cnt < k) {  // (at most two bytes a call: bounded by the input)
    if (b.pos == b.blk_end && !gif_hop(b)) return false;
    b.buf |= (uint64_t)(uint32_t)b.rd(b.pos++) << b.cnt;
    b.cnt += 8;
  }
  *v = (uint32_t)(b.buf & ((1ull << k) - 1));
  b.buf >>= k;
  b.cnt -= k;
  return true;
}

// The LZW table: entry c (above the end code) is a string that already stands in the output, at off[c],
// len[c] bytes long.  The entry a code makes is the previous code's string plus the first byte of its own,
// and the two are neighbours in the output, so an entry is (the previous string's offset, its length + 1)
// and costs no byte of storage.  24 KiB: the device keeps it in LDS.
struct GifTable {
  uint32_t off[kGifTable];
  uint16_t len[kGifTable];
};

// The frame's `expect` index bytes into `out` (the sinks of sdsj_png_wave.h and tests/asan/gif_driver.cpp):
//   out.lit(byte)          appends one byte
//   out.match(dist, len)   appends len bytes copied from dist bytes back (overlap allowed: the KwKwK case
//                          copies its own first byte)
// The sink never sees a byte beyond `expect` or a source before the first byte.  Every code is read with
// gif_take, so the loop is bounded by the input's length, and it ends at `expect` bytes.  SDSJ_OK: exactly
// `expect` bytes were produced (whatever follows is not read); SDSJ_CORRUPT: an end code or the end of the
// chain before that, a sub-block past the input, a code above the next free entry, a first code after a
// clear that is not a literal.
template <class Reader, class Sink>
SDSJ_HDI int gif_lzw(GifBits<Reader>& b, GifTable* T, Sink& out, int64_t expect, int min_code) {
  if (min_code < 2 || min_code > 8 || expect <= 0) return SDSJ_CORRUPT;
  const int clear = 1 << min_code, end = clear + 1;
  int next = clear + 2, size = min_code + 1, mask = (1 << size) - 1;
  int last = -1;            // the previous code (-1: none since the clear)
  int64_t prev_pos = 0;     // where its string stands in the output
  int prev_len = 0;
  int64_t produced = 0;
  while (produced < expect) {
    uint32_t v;
    if (!gif_take(b, size, &v)) return SDSJ_CORRUPT;
    const int c = (int)v;
    if (c == clear) {
      next = clear + 2;
      size = min_code + 1;
      mask = (1 << size) - 1;
      last = -1;
      continue;
    }
    if (c == end) return SDSJ_CORRUPT;
    int64_t src = -1;  // the string's offset; -1: the literal c
    int len = 1;
    if (last < 0) {
      if (c > clear) return SDSJ_CORRUPT;
    } else if (c >= clear) {
      if (c > next || c >= kGifTable) return SDSJ_CORRUPT;  // (a full table has no next entry)
      if (c == next) {
        if (next >= kGifTable) return SDSJ_CORRUPT;
        src = prev_pos;
        len = prev_len + 1;
      } else {
        src = (int64_t)T->off[c];
        len = (int)T->len[c];
      }
    }
    const int64_t room = expect - produced;
    const int emit = (int64_t)len < room ? len : (int)room;
    if (src < 0) {
      out.lit(c);
    } else {
      const int64_t dist = produced - src;
      // (cannot fail: an entry's string ends at or before `produced`; checked because a copy follows)
      if (dist < 1 || dist > produced || dist > 0x7FFFFFFF || emit < 1) return SDSJ_CORRUPT;
      out.match((int)dist, emit);
    }
    if (last >= 0 && next < kGifTable) {
      T->off[next] = (uint32_t)prev_pos;
      T->len[next] = (uint16_t)(prev_len + 1);
      if (next == mask && size < 12) {
        size++;
        mask = (1 << size) - 1;
      }
      next++;
    }
    last = c;
    prev_pos = produced;
    prev_len = len;
    produced += emit;
  }
  return SDSJ_OK;
}

}  // namespace sdsj
