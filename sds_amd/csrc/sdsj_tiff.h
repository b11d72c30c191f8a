// sdsj_tiff.h -- the TIFF subset the MI355X path decodes (SDSJ_FORMAT_TIFF), as functions shared by the host
// (sdsj_tiff_probe, host planning, the serial decoder of tests/asan/tiff_driver.cpp) and the device (k_parse,
// k_tiff_copy, k_tiff_lzw, k_tiff_inflate, k_tiff_rgb in sdsj_tiff.hip).  Every decision about correctness or
// bounds is taken here; the kernels add only the lane-parallel movement of bytes.
//
// Reference behaviour: PIL.Image.open(...).convert("RGB") (TiffImagePlugin.py, Pillow 12.2.0: uncompressed strips
// through its own raw decoder, compressed ones through libtiff 4.7.1), the first IFD.  What synthesised files
// (tests/tiff_synth.py, pinned by tests/test_tiff_host.py) settled:
//   - photometric 0 inverts: a grey sample s opens as 255 - s; photometric 1 as s
//   - a ColorMap entry of 16 bits becomes 8 by dropping its low byte (v >> 8), not by rounding v / 257
//   - CMYK is Convert.c cmyk2rgb, ((255 - ink) * (255 - k) + 127) / 255 per channel; the extra sample of an
//     RGB file (ExtraSamples 2 or 0) and of a grey one (photometric 1, ExtraSamples 2) is dropped without compositing
//   - uncompressed strips: PIL reads rows x width x samples bytes at each offset and never looks at
//     StripByteCounts, so a count beyond the file or below the strip's size still opens.  This path asks for a
//     count inside the file that covers the strip (SDSJ_CORRUPT otherwise: PIL decides)
//   - compressed strips stop at the strip's size: LZW needs no end code and bytes after it are not read;
//     Deflate output beyond the strip's rows is dropped by libtiff without an error, and so is a PackBits run
//     that crosses the strip's end.  Both are refused here (SDSJ_CORRUPT: doubtful), as is a stream that
//     is cut before its Adler-32, which libtiff lets pass.  A strip that decodes to fewer bytes (an early end code,
//     a short Deflate stream, PackBits data that ends), a wrong Adler-32 or zlib header, an LZW code above the
//     next free entry and a first code that is no clear code raise in PIL: SDSJ_CORRUPT
//   - PackBits: the byte 0x80 is skipped wherever a run could start; a run may cross a row inside its strip
//   - strips may lie in any order in the file, with gaps or overlaps between them: each is read on its own
//   - a missing StripByteCounts or StripOffsets raises; StripByteCounts of another length than StripOffsets
//     raises, and so do fewer strips than the rows need
//   - tags out of order still open in this Pillow, and so does a ColorMap of 96 entries or an unknown tag whose
//     value lies past the file; libtiff's own directory reader is involved for compressed files, so all three
//     are SDSJ_CORRUPT here (PIL decides).  A palette file without ColorMap, a zero width, RowsPerStrip 0 and a
//     BitsPerSample count that differs from SamplesPerPixel raise
//   - a grey file with an extra sample opens only as photometric 1 with ExtraSamples 2 ("LA"); photometric 0 with
//     either kind and photometric 1 with kind 0 raise UnidentifiedImageError: SDSJ_UNSUPPORTED.  RGB opens with both
//   - RowsPerStrip above the height is fine up to 0x7FFFFFFF and as 0xFFFFFFFF; 0x80000000..0xFFFFFFFE raise for
//     compressed files (uncompressed ones open): SDSJ_CORRUPT for all
//   - libtiff fails on tags it knows with a type or count it rejects (tags 280 / 281 as RATIONALs, 340 / 341 as
//     ASCII make an LZW file raise), so tags beside the layout pass only from a short list, each with its type and
//     count (tiff_passive_tag_ok); a file with any other tag is SDSJ_CORRUPT (PIL decides).  Duplicate tags: as
//     unsorted ones
//   - SampleFormat opens with one value or one per sample; another count (2 values for 3 samples) raises for
//     compressed files: SDSJ_CORRUPT for all
//   - orientation 2..8 is applied at open (a 7 x 5 file with orientation 6 opens as 5 x 7): SDSJ_UNSUPPORTED
// The rule is exactness, as for PNG, GIF and WebP: SDSJ_OK only where PIL decodes the same bytes to the same
// pixels without raising; a valid file outside the subset is SDSJ_UNSUPPORTED, anything malformed or unsure
// SDSJ_CORRUPT, and the transforms rerun both on PIL, which then decides.
#pragma once
#include <stdint.h>

#include "sdsj_common.h"
#include "sdsj_gif.h"  // GifTable: the LZW table's layout
#include "sdsj_png.h"  // SDSJ_HDI, kPngMaxPixels, kPngMaxRaw, the inflate tables and bit reader

namespace sdsj {

constexpr int kTiffSample = 4;         // ImgDesc::png of a TIFF sample
constexpr int kTiffMaxEntries = 512;   // IFD entries this path walks
constexpr int kTiffMaxStrips = 65536;  // strips of one image
enum TiffCodec : int32_t { kTiffNone = 1, kTiffPackBits = 2, kTiffLzw = 3, kTiffDeflate = 4 };

struct TiffHdr {
  int32_t width, height;
  int32_t codec;       // TiffCodec
  int32_t predictor;   // 1 or 2
  int32_t photo;       // 0, 1, 2, 3, 5
  int32_t spp;         // samples per pixel as stored (an extra sample included)
  int32_t rps;         // rows per strip, at most the height
  int32_t nstrips;
  int32_t be;          // 1: MM
  int32_t off_long, cnt_long;  // 1: LONG entries, 0: SHORT
  int64_t off_pos, cnt_pos, cmap_pos;  // first byte of the StripOffsets / StripByteCounts / ColorMap values
};

template <class Reader>
SDSJ_HD inline bool tiff_signature(const Reader& rd, int64_t n) {  // classic TIFF or BigTIFF (refused by the parse)
  if (n < 4) return false;
  if (rd(0) == 'I' && rd(1) == 'I') return (rd(2) == 42 || rd(2) == 43) && rd(3) == 0;
  if (rd(0) == 'M' && rd(1) == 'M') return rd(2) == 0 && (rd(3) == 42 || rd(3) == 43);
  return false;
}

template <class Reader>
SDSJ_HDI uint32_t tiff_u16(const Reader& rd, int64_t i, int be) {
  const uint32_t a = (uint32_t)rd(i), b = (uint32_t)rd(i + 1);
  return be ? (a << 8) | b : a | (b << 8);
}
template <class Reader>
SDSJ_HDI uint32_t tiff_u32(const Reader& rd, int64_t i, int be) {
  const uint32_t a = tiff_u16(rd, i, be), b = tiff_u16(rd, i + 2, be);
  return be ? (a << 16) | b : a | (b << 16);
}
// Value k of a SHORT (is_long == 0) or LONG array at p.
template <class Reader>
SDSJ_HDI uint32_t tiff_value(const Reader& rd, int64_t p, int is_long, int64_t k, int be) {
  return is_long ? tiff_u32(rd, p + 4 * k, be) : tiff_u16(rd, p + 2 * k, be);
}
SDSJ_HD inline int tiff_type_size(int type) {  // 0: a type this path does not know
  switch (type) {
    case 1: case 2: case 6: case 7: return 1;
    case 3: case 8: return 2;
    case 4: case 9: case 11: case 13: return 4;
    case 5: case 10: case 12: return 8;
    default: return 0;
  }
}

// The tags beside the layout that this path lets pass, each with the type and count libtiff wants: NewSubfileType,
// the ASCII descriptions, the resolution, XMP, the ICC profile, and the reusable private range 65000..65535, which
// libtiff has no definition for and takes as it comes.
SDSJ_HD inline bool tiff_passive_tag_ok(int tag, int type, int64_t count) {
  if (count < 1) return false;
  switch (tag) {
    case 254: return type == 4 && count == 1;
    case 270: case 271: case 272: case 305: case 315: return type == 2;
    case 306: return type == 2 && count == 20;
    case 282: case 283: return type == 5 && count == 1;
    case 296: return type == 3 && count == 1;
    case 700: return type == 1 || type == 7;
    case 34675: return type == 7;
    default: return tag >= 65000;
  }
}

// One strip of a parsed file: its bytes [pos, pos + len) in the sample, its first row, its rows and the bytes
// they take (rows x width x samples).
struct TiffStrip {
  int64_t pos, len;
  int32_t row0, rows;
  int64_t expect;
};

// What the kernels need of a TIFF descriptor (tiff_fill_desc packs it into the PNG fields).
struct TiffView {
  int32_t codec, predictor, photo, spp, rps, nstrips, be, off_long, cnt_long;
  int64_t off_pos, cnt_pos, cmap_pos;
};

// Strip s (0 .. nstrips - 1) from the StripOffsets / StripByteCounts values in the sample's bytes.  False
// where it leaves the sample or cannot hold its rows (tiff_parse has checked every strip: the kernels check again
// because they read what this returns).
template <class Reader>
SDSJ_HD inline bool tiff_strip(const Reader& rd, int64_t n, const TiffView& v, int width, int height, int s, TiffStrip* out) {
  if (s < 0 || s >= v.nstrips || v.rps < 1) return false;
  const int64_t row0 = (int64_t)s * v.rps;
  if (row0 >= height) return false;
  const int64_t rows = height - row0 < v.rps ? height - row0 : v.rps;
  const int64_t unit_o = v.off_long ? 4 : 2, unit_c = v.cnt_long ? 4 : 2;
  if (v.off_pos < 0 || v.cnt_pos < 0 || v.off_pos + unit_o * (s + 1) > n || v.cnt_pos + unit_c * (s + 1) > n) return false;
  out->pos = (int64_t)tiff_value(rd, v.off_pos, v.off_long, s, v.be);
  out->len = (int64_t)tiff_value(rd, v.cnt_pos, v.cnt_long, s, v.be);
  out->row0 = (int32_t)row0;
  out->rows = (int32_t)rows;
  out->expect = rows * width * v.spp;
  if (out->len < 1 || out->pos < 8 || out->pos > n || out->len > n - out->pos) return false;
  if (v.codec == kTiffNone && out->len < out->expect) return false;
  return true;
}

// Header, the first IFD and every strip's range.  h's size is filled as soon as it has been read, whatever the
// status.  The entry count is bounded; every offset and every count x size is checked against the input's length
// in 64 bits (a count is below 2^32 and a size at most 8).  No byte outside [0, n) is read.
template <class Reader>
SDSJ_HD int tiff_parse(const Reader& rd, int64_t n, TiffHdr* h) {
  h->width = h->height = h->codec = h->photo = h->spp = h->rps = h->nstrips = h->be = h->off_long = h->cnt_long = 0;
  h->predictor = 1;
  h->off_pos = h->cnt_pos = h->cmap_pos = 0;
  if (!tiff_signature(rd, n)) return SDSJ_UNSUPPORTED;
  const int be = rd(0) == 'M';
  h->be = be;
  if (tiff_u16(rd, 2, be) != 42u) return SDSJ_UNSUPPORTED;  // BigTIFF
  if (n < 8) return SDSJ_CORRUPT;
  const int64_t ifd = (int64_t)tiff_u32(rd, 4, be);
  if (ifd < 8 || ifd + 2 > n) return SDSJ_CORRUPT;
  const int entries = (int)tiff_u16(rd, ifd, be);
  if (entries == 0) return SDSJ_CORRUPT;
  if (entries > kTiffMaxEntries) return SDSJ_UNSUPPORTED;
  if (ifd + 2 + (int64_t)12 * entries + 4 > n) return SDSJ_CORRUPT;  // (the next-IFD offset included)
  bool unsup = false;
  int64_t width = -1, height = -1, rps = 0xFFFFFFFFll, off_cnt = -1, cnt_cnt = -1, cmap_cnt = -1;
  int comp = 1, photo = -1, spp = 1, bps_n = 0, sf_n = 0, extra_n = 0, extra0 = 0, predictor = 1, cmap_type = 0;
  int off_type = 0, cnt_type = 0;
  int last_tag = -1;
  for (int k = 0; k < entries; k++) {
    const int64_t e = ifd + 2 + (int64_t)12 * k;
    const int tag = (int)tiff_u16(rd, e, be), type = (int)tiff_u16(rd, e + 2, be);
    const int64_t count = (int64_t)tiff_u32(rd, e + 4, be);
    if (tag <= last_tag) return SDSJ_CORRUPT;  // duplicate or unsorted tags
    last_tag = tag;
    const int size = tiff_type_size(type);
    if (size == 0) return SDSJ_CORRUPT;
    const int64_t bytes = count * size;
    int64_t pos = e + 8;
    if (bytes > 4) {
      pos = (int64_t)tiff_u32(rd, e + 8, be);
      if (pos < 8 || pos > n || bytes > n - pos) return SDSJ_CORRUPT;
    }
    const bool num = type == 3 || type == 4;  // SHORT or LONG
    const uint32_t v0 = num && count >= 1 ? tiff_value(rd, pos, type == 4, 0, be) : 0u;
    switch (tag) {
      case 256: case 257: case 259: case 262: case 266: case 274: case 277: case 278: case 284: case 317:
        if (!num || count != 1) return SDSJ_CORRUPT;
        if (tag == 256) width = v0, h->width = v0 <= 0x7FFFFFFFu ? (int32_t)v0 : 0;
        if (tag == 257) height = v0, h->height = v0 <= 0x7FFFFFFFu ? (int32_t)v0 : 0;
        if (tag == 259) comp = v0 <= 0xFFFFu ? (int)v0 : 0;
        if (tag == 262) photo = v0 <= 0xFFFFu ? (int)v0 : 0xFFFF;
        if (tag == 266 && v0 != 1u) unsup = true;
        if (tag == 274 && v0 != 1u) unsup = true;
        if (tag == 277) spp = v0 <= 64u ? (int)v0 : 65;
        if (tag == 278) rps = v0;
        if (tag == 284 && v0 != 1u) unsup = true;
        if (tag == 317) predictor = v0 <= 0xFFFFu ? (int)v0 : 0;
        break;
      case 258: case 339:  // BitsPerSample: 8 for every sample; SampleFormat: unsigned integers
        if (!num || count < 1) return SDSJ_CORRUPT;
        if (count > 8) {
          unsup = true;
        } else {
          for (int64_t i = 0; i < count; i++)
            if (tiff_value(rd, pos, type == 4, i, be) != (tag == 258 ? 8u : 1u)) unsup = true;
        }
        if (tag == 258) bps_n = count > 8 ? 9 : (int)count;
        else sf_n = count > 8 ? 9 : (int)count;
        break;
      case 273:
        if (!num || count < 1) return SDSJ_CORRUPT;
        off_type = type, off_cnt = count, h->off_pos = pos;
        break;
      case 279:
        if (!num || count < 1) return SDSJ_CORRUPT;
        cnt_type = type, cnt_cnt = count, h->cnt_pos = pos;
        break;
      case 320:
        cmap_type = type, cmap_cnt = count, h->cmap_pos = pos;
        break;
      case 338:
        if (!num || count < 1) return SDSJ_CORRUPT;
        extra_n = count > 8 ? 9 : (int)count;
        extra0 = v0 <= 0xFFFFu ? (int)v0 : 0xFFFF;
        break;
      case 322: case 323: case 324: case 325:  // tiles
        unsup = true;
        break;
      case 332:  // InkSet: CMYK only
        if (!num || count != 1) return SDSJ_CORRUPT;
        if (v0 != 1u) unsup = true;
        break;
      default:
        // libtiff reads the whole directory of a compressed file and fails on tags it knows whose type or count it
        // rejects (a RATIONAL MinSampleValue, an ASCII SMinSampleValue), so only tags checked against it pass, with
        // the type and count it wants; none of them reaches the pixels of convert("RGB").  Every other tag: PIL decides
        if (!tiff_passive_tag_ok(tag, type, count)) return SDSJ_CORRUPT;
        break;
    }
  }
  if (width < 1 || height < 1) return SDSJ_CORRUPT;
  if (width > 0x7FFFFFFF || height > 0x7FFFFFFF || width * height > kPngMaxPixels) return SDSJ_UNSUPPORTED;
  if (unsup) return SDSJ_UNSUPPORTED;
  if (photo < 0 || bps_n == 0) return SDSJ_UNSUPPORTED;  // (the defaults are bilevel)
  if (spp < 1 || spp > 64) return SDSJ_UNSUPPORTED;
  int base = 0;
  if (photo == 0 || photo == 1 || photo == 3) base = 1;
  else if (photo == 2) base = 3;
  else if (photo == 5) base = 4;
  else return SDSJ_UNSUPPORTED;
  if (spp < base || spp > base + 1) return SDSJ_UNSUPPORTED;  // fewer samples than the colour space, several extras
  if (spp == base + 1 && (photo == 3 || photo == 5)) return SDSJ_UNSUPPORTED;
  if (spp == base + 1 && extra_n == 0) return SDSJ_UNSUPPORTED;  // (PIL guesses what the fourth sample is)
  if (bps_n != spp) return SDSJ_CORRUPT;
  // (libtiff reads SampleFormat per sample: one value for all, or one each; it fails the directory on other counts)
  if (sf_n != 0 && sf_n != 1 && sf_n != spp) return SDSJ_CORRUPT;
  if (extra_n != spp - base) return SDSJ_CORRUPT;
  if (extra_n == 1 && extra0 != 0 && extra0 != 2) return SDSJ_UNSUPPORTED;  // associated alpha opens premultiplied
  // (PIL's table of modes has one grey file with an extra sample: photometric 1 with unassociated alpha, "LA")
  if (extra_n == 1 && base == 1 && !(photo == 1 && extra0 == 2)) return SDSJ_UNSUPPORTED;
  int codec = 0;
  if (comp == 1) codec = kTiffNone;
  else if (comp == 32773) codec = kTiffPackBits;
  else if (comp == 5) codec = kTiffLzw;
  else if (comp == 8 || comp == 32946) codec = kTiffDeflate;
  else return SDSJ_UNSUPPORTED;
  if (predictor != 1 && !(predictor == 2 && (codec == kTiffLzw || codec == kTiffDeflate))) return SDSJ_UNSUPPORTED;
  if (photo == 3) {
    if (cmap_cnt < 0 || cmap_type != 3 || cmap_cnt != 768) return SDSJ_CORRUPT;
  }
  if ((int64_t)width * height * spp > kPngMaxRaw) return SDSJ_UNSUPPORTED;
  if (off_cnt < 0 || cnt_cnt < 0 || off_cnt != cnt_cnt) return SDSJ_CORRUPT;
  if (rps < 1) return SDSJ_CORRUPT;
  if (rps > 0x7FFFFFFFll && rps != 0xFFFFFFFFll) return SDSJ_CORRUPT;  // (libtiff raises on these for compressed files)
  if (rps > height) rps = height;
  const int64_t nstrips = (height + rps - 1) / rps;
  if (off_cnt != nstrips) return SDSJ_CORRUPT;
  if (nstrips > kTiffMaxStrips) return SDSJ_UNSUPPORTED;
  h->codec = codec;
  h->predictor = predictor;
  h->photo = photo;
  h->spp = spp;
  h->rps = (int32_t)rps;
  h->nstrips = (int32_t)nstrips;
  h->off_long = off_type == 4;
  h->cnt_long = cnt_type == 4;
  const TiffView v{codec, predictor, photo, spp, h->rps, h->nstrips, be, h->off_long, h->cnt_long, h->off_pos, h->cnt_pos, h->cmap_pos};
  for (int s = 0; s < h->nstrips; s++) {
    TiffStrip st;
    if (!tiff_strip(rd, n, v, h->width, h->height, s, &st)) return SDSJ_CORRUPT;
    // old-style LZW (codes LSB first, as libtiff's LZWDecodeCompat tells it): outside the subset
    if (s == 0 && codec == kTiffLzw && st.len >= 2 && rd(st.pos) == 0 && (rd(st.pos + 1) & 1)) return SDSJ_UNSUPPORTED;
  }
  return SDSJ_OK;
}

SDSJ_HD inline TiffView tiff_view(const ImgDesc& d) {
  const uint32_t f = (uint32_t)d.png_depth_lace;
  return TiffView{(int32_t)(f & 7u), (int32_t)((f >> 3) & 1u) + 1, (int32_t)((f >> 4) & 15u), d.png_bpp, d.png_ctype,
                  d.png_plte_n, (int32_t)((f >> 8) & 1u), (int32_t)((f >> 9) & 1u), (int32_t)((f >> 10) & 1u),
                  (int64_t)((uint64_t)d.png_idat_pos & 0xFFFFFFFFull), (int64_t)((uint64_t)d.png_idat_pos >> 32), d.png_plte_pos};
}

// The descriptor of a parsed TIFF: like a PNG's it has no components, blocks or entropy data, and neither the PNG,
// the GIF nor the WebP kernels meet it (its route is kRtTiff; they test png == 1 / 2 / 3).  ImgDesc keeps its size
// and offsets, and everything the kernels need fits the PNG fields, so no record goes to the scratch:
//   png_ctype      rows per strip (at most the height)
//   png_bpp        samples per pixel as stored
//   png_plte_n     strips
//   png_plte_pos   first byte of the ColorMap values (3 x 256 SHORTs), relative to the sample's first byte
//   png_idat_pos   first byte of the StripOffsets values | first byte of the StripByteCounts values << 32 (a
//                  sample is shorter than 2^31 bytes)
//   png_raw        height x width x samples: the decoded strips at off_png, each at its first row's place
//   png_depth_lace codec (TiffCodec) | (predictor - 1) << 3 | photometric << 4 | byte order (1: MM) << 8 |
//                  StripOffsets are LONGs << 9 | StripByteCounts are LONGs << 10
SDSJ_HD inline void tiff_fill_desc(ImgDesc* d, const TiffHdr& h) {
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
  d->png = kTiffSample;
  d->png_ctype = h.rps;
  d->png_bpp = h.spp;
  d->png_plte_n = h.nstrips;
  d->png_plte_pos = h.cmap_pos;
  d->png_idat_pos = (int64_t)(((uint64_t)h.off_pos & 0xFFFFFFFFull) | ((uint64_t)h.cnt_pos << 32));
  d->png_raw = (int64_t)h.width * h.height * h.spp;
  d->png_depth_lace = (h.codec & 7) | (((h.predictor - 1) & 1) << 3) | ((h.photo & 15) << 4) | ((h.be & 1) << 8) |
                      ((h.off_long & 1) << 9) | ((h.cnt_long & 1) << 10);
  d->off_png = 0;
}

// ------------------------------------------------------------------------------------------
// PackBits.  The control bytes are read through `rd`; the runs go to the sink:
//   out.copy(src, k)   appends the input's bytes [src, src + k)
//   out.fill(b, k)     appends k bytes b
// SDSJ_OK: exactly `expect` bytes were produced from [p, e) (what follows is not read).  SDSJ_CORRUPT: the data
// ends first, or a run crosses the strip's end.  The sink never sees a byte beyond `expect` or an input
// byte outside [p, e).
// ------------------------------------------------------------------------------------------
template <class Reader, class Sink>
SDSJ_HDI int tiff_packbits(const Reader& rd, int64_t p, int64_t e, Sink& out, int64_t expect) {
  int64_t produced = 0;
  while (produced < expect) {
    if (p >= e) return SDSJ_CORRUPT;
    const int c = rd(p++);
    if (c == 128) continue;  // the no-op
    if (c < 128) {
      const int k = c + 1;
      if (k > e - p || k > expect - produced) return SDSJ_CORRUPT;
      out.copy(p, k);
      p += k;
      produced += k;
    } else {
      const int k = 257 - c;
      if (p >= e || k > expect - produced) return SDSJ_CORRUPT;
      out.fill(rd(p++), k);
      produced += k;
    }
  }
  return SDSJ_OK;
}

// ------------------------------------------------------------------------------------------
// LZW as TIFF has it: codes MSB first, 9 to 12 bits, the width growing one code early (when the next free entry
// is 511, 1023, 2047), clear 256, end-of-information 257, entries from 258.
// ------------------------------------------------------------------------------------------
template <class Reader>
struct TiffBits {
  Reader rd;  // (by value, as in GifBits)
  int64_t pos, end;
  uint32_t buf;
  int32_t cnt;
};

template <class Reader>
SDSJ_HDI void tiff_bits_init(TiffBits<Reader>& b, const Reader& rd, int64_t p, int64_t e) {
  b.rd = rd;
  b.pos = p;
  b.end = e;
  b.buf = 0;
  b.cnt = 0;
}

template <class Reader>
SDSJ_HDI bool tiff_take(TiffBits<Reader>& b, int k, uint32_t* v) {  // k <= 12 bits; false: data exhausted
  while (b.cnt < k) {
    if (b.pos >= b.end) return false;
    b.buf = (b.buf << 8) | (uint32_t)b.rd(b.pos++);
    b.cnt += 8;
  }
  *v = (b.buf >> (b.cnt - k)) & ((1u << k) - 1);
  b.cnt -= k;
  return true;
}

// The strip's `expect` bytes into `out` (lit / match, as gif_lzw's sink; the table is gif_lzw's too: an entry is
// where its string already stands in the strip's output).  SDSJ_OK: exactly `expect` bytes were produced (a
// string that would pass them is cut there, as LZWDecode does; what follows is not read).  SDSJ_CORRUPT: a first
// code that is no clear code, an end code or the end of the data before that, a code above the next free entry,
// a first code after a clear that is no literal, and a table that would take entry 4095 (writers clear at 4094).
template <class Reader, class Sink>
SDSJ_HDI int tiff_lzw(TiffBits<Reader>& b, GifTable* T, Sink& out, int64_t expect) {
  if (expect <= 0) return SDSJ_CORRUPT;
  const int clear = 256, end = 257;
  int next = 258, size = 9, mask = 511;
  int last = -1;
  bool first = true;
  int64_t prev_pos = 0;
  int prev_len = 0;
  int64_t produced = 0;
  while (produced < expect) {
    uint32_t v;
    if (!tiff_take(b, size, &v)) return SDSJ_CORRUPT;
    const int c = (int)v;
    if (first && c != clear) return SDSJ_CORRUPT;
    first = false;
    if (c == clear) {
      next = 258;
      size = 9;
      mask = 511;
      last = -1;
      continue;
    }
    if (c == end) return SDSJ_CORRUPT;
    int64_t src = -1;  // the string's offset; -1: the literal c
    int len = 1;
    if (last < 0) {
      if (c > 255) return SDSJ_CORRUPT;
    } else if (c > 255) {
      if (c > next || c >= kGifTable - 1) return SDSJ_CORRUPT;
      if (c == next) {
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
      if (dist < 1 || dist > produced || dist > 0x7FFFFFFF || emit < 1) return SDSJ_CORRUPT;
      out.match((int)dist, emit);
    }
    if (last >= 0) {
      if (next >= kGifTable - 1) return SDSJ_CORRUPT;
      T->off[next] = (uint32_t)prev_pos;
      T->len[next] = (uint16_t)(prev_len + 1);
      next++;
      if (next == mask && size < 12) {  // the early change
        size++;
        mask = (1 << size) - 1;
      }
    }
    last = c;
    prev_pos = produced;
    prev_len = len;
    produced += emit;
  }
  return SDSJ_OK;
}

// ------------------------------------------------------------------------------------------
// Deflate: the strip form of png_inflate -- one contiguous range (a reader made by png_bits_span) instead of an
// IDAT chain, the same tables, bit reader and sink.  SDSJ_OK: a well-formed zlib stream that ends in a final
// block after exactly `expect` bytes and whose Adler-32 lies inside the range; *adler = the trailer's value (the
// caller compares it with the output's).  Bytes after the trailer are not read.
// ------------------------------------------------------------------------------------------
template <class Reader, class Sink>
SDSJ_HDI int tiff_inflate(PngBits<Reader>& b, InfTables* T, Sink& out, int64_t expect, uint32_t* adler) {
  int window = 0;
  if (!zlib_header(b, &window)) return SDSJ_CORRUPT;
  int64_t produced = 0;
  for (;;) {
    int final = 0, type = 0, stored = 0;
    if (!inf_block_header(b, T, &final, &type, &stored)) return SDSJ_CORRUPT;
    if (type == 0) {
      if (produced + stored > expect) return SDSJ_CORRUPT;
      for (int k = 0; k < stored; k++) {
        uint32_t v;
        if (!png_take(b, 8, &v)) return SDSJ_CORRUPT;
        out.lit((int)v);
      }
      produced += stored;
    } else {
      for (;;) {
        const int s = inf_decode(b, &T->ll, T->ll_sym);
        if (s < 0) return SDSJ_CORRUPT;
        if (s < 256) {
          if (produced >= expect) return SDSJ_CORRUPT;
          out.lit(s);
          produced++;
          continue;
        }
        if (s == 256) break;
        int len = 0, dist = 0;
        if (!inf_length(b, s, &len) || !inf_distance(b, T, &dist)) return SDSJ_CORRUPT;
        if (!inf_match_ok(produced, expect, dist, len, window)) return SDSJ_CORRUPT;
        out.match(dist, len);
        produced += len;
      }
    }
    if (final) break;
  }
  if (produced != expect) return SDSJ_CORRUPT;
  const int drop = b.cnt & 7;
  b.buf >>= drop;
  b.cnt -= drop;
  uint32_t v;
  if (!png_take(b, 32, &v)) return SDSJ_CORRUPT;
  *adler = ((v & 0xFF) << 24) | ((v & 0xFF00) << 8) | ((v >> 8) & 0xFF00) | (v >> 24);
  return SDSJ_OK;
}

// ------------------------------------------------------------------------------------------
// Predictor 2 and the pixel of convert("RGB").  A pixel travels as its samples packed little-endian in a dword
// (spp <= 4).
// ------------------------------------------------------------------------------------------
// Horizontal differencing undone for one pixel: its stored samples plus those of the finished pixel to its left,
// per byte, modulo 256.  The sum is associative, so the device takes a row's prefix sums by waves (k_tiff_rgb); the
// sanitizer driver walks the row.
SDSJ_HD inline uint32_t tiff_unpredict(uint32_t a, uint32_t b) {
  const uint32_t even = ((a & 0x00FF00FFu) + (b & 0x00FF00FFu)) & 0x00FF00FFu;
  const uint32_t odd = (((a >> 8) & 0x00FF00FFu) + ((b >> 8) & 0x00FF00FFu)) & 0x00FF00FFu;
  return even | (odd << 8);
}

// r | g << 8 | b << 16 of a pixel's samples; `cmap(i)` returns byte i of the ColorMap values (3 x 256 SHORTs in the
// file's byte order: the high byte of each is the colour).
template <class Pal>
SDSJ_HD inline uint32_t tiff_rgb(uint32_t px, int photo, int be, const Pal& cmap) {
  const uint32_t s0 = px & 255u;
  if (photo == 2) return px & 0xFFFFFFu;
  if (photo == 1) return s0 * 0x010101u;
  if (photo == 0) return (255u - s0) * 0x010101u;
  if (photo == 3) {
    const int hi = be ? 0 : 1;
    return (uint32_t)cmap(2 * (int)s0 + hi) | ((uint32_t)cmap(512 + 2 * (int)s0 + hi) << 8) | ((uint32_t)cmap(1024 + 2 * (int)s0 + hi) << 16);
  }
  // CMYK, inks not inverted (Convert.c cmyk2rgb)
  const uint32_t k = 255u - (px >> 24);
  const uint32_t r = ((255u - s0) * k + 127u) / 255u, g = ((255u - ((px >> 8) & 255u)) * k + 127u) / 255u,
                 bl = ((255u - ((px >> 16) & 255u)) * k + 127u) / 255u;
  return r | (g << 8) | (bl << 16);
}

}  // namespace sdsj
