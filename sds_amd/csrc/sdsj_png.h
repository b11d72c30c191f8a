// sdsj_png.h -- the PNG subset the MI355X path decodes, as functions shared by the host (sdsj_png_probe,
// host planning, the serial decoder of tests/asan/png_driver.cpp) and the device (k_parse,
// k_png_inflate, k_png_unfilter in sdsj_png.hip).  Every decision about correctness or bounds is taken
// here; the kernels add only the lane-parallel movement of bytes.
//
// Reference behaviour: PIL.Image.open(...).convert("RGB") (PngImagePlugin.py + ZipDecode.c + zlib).
// Subset: non-interlaced, bit depth 8, colour types 0, 2, 3, 4, 6; with SDSJ_FORMAT_PNG_EXT in the mask
// also Adam7 interlace, bit depths 1, 2, 4 and 16 and more ancillary chunks before the image data
// (png_parse's `formats`, png_layout, the 64-bit png_recon, png_rgb_ext); with SDSJ_FORMAT_PNG_META also
// iCCP, zTXt and iTXt chunks and chunks after the image data (png_meta_check).  The rule is exactness: a sample is
// reported SDSJ_OK only where PIL decodes the same bytes to the same pixels without raising; everything
// this code is not sure about is SDSJ_UNSUPPORTED (a valid file outside the subset) or SDSJ_CORRUPT
// (anything malformed), and the transforms rerun both on PIL, which then decides.
#pragma once
#include <stdint.h>

#include "sdsj_common.h"

// Functions that take the bit reader are inlined into the kernel: its state then lives in registers
// (a call would keep it in memory behind a reference).
#if defined(__HIPCC__)
#define SDSJ_HDI __host__ __device__ __attribute__((always_inline)) inline
#else
#define SDSJ_HDI inline
#endif

namespace sdsj {

struct PngHdr {
  int32_t width, height, bit_depth, ctype, interlace;
  int32_t bpp;       // the filter unit: bytes per pixel of the scanlines, 1 for depths below 8 (png_unit)
  int32_t plte_n;    // PLTE entries (0: none)
  int32_t zero;
  int64_t plte_pos;  // first PLTE data byte
  int64_t idat_pos;  // length field of the first IDAT chunk
};

constexpr int64_t kPngMaxPixels = 89478485;      // PIL Image.MAX_IMAGE_PIXELS: above it Image.open warns or raises
constexpr int64_t kPngMaxHeader = 1 << 20;       // bytes before the first IDAT this path walks
constexpr int64_t kPngMaxRaw = (int64_t)1 << 30;  // inflated scanline bytes of one image

// ------------------------------------------------------------------------------------------
// Scanline layout (PNG specification 7.2, 8.2, 9.2).  The filter unit is the whole bytes of a pixel,
// 1 for depths below 8.  A non-interlaced image is one pass; an Adam7 image has up to seven, each a
// complete filtered image of its own (pass width x pass height, its upper row starting as zeros), and
// a pass without columns or rows contributes no bytes at all, not even filter bytes.
// ------------------------------------------------------------------------------------------
SDSJ_HD inline int png_channels(int ctype) { return ctype == 2 ? 3 : ctype == 4 ? 2 : ctype == 6 ? 4 : 1; }
SDSJ_HD inline int png_unit(int ctype, int depth) {
  const int u = png_channels(ctype) * depth / 8;
  return u < 1 ? 1 : u;
}

struct PngPass {
  int32_t xs, ys, dx, dy;  // image x = xs + px * dx, y = ys + py * dy
  int32_t w, h;            // pass size in pixels
  int64_t rowbytes;        // ceil(w * bits per pixel / 8), without the filter byte
  int64_t off;             // first byte (row 0's filter byte) of the pass in the inflated buffer
};

// Geometry of pass `slot` (0: the whole image of a non-interlaced file; 0..6: the Adam7 passes) and the
// bytes of the passes before it; false: the pass is empty.  No table in memory: the kernels call this
// with a wave-uniform slot.
SDSJ_HD inline bool png_pass_at(int w, int h, int ctype, int depth, int interlace, int slot, PngPass* ps) {
  const int64_t bits = (int64_t)png_channels(ctype) * depth;
  const int np = interlace ? 7 : 1;
  int64_t off = 0;
  for (int p = 0; p < np; p++) {
    // (x start, y start, x step, y step) of the Adam7 passes: 0,0,8,8  4,0,8,8  0,4,4,8  2,0,4,4  0,2,2,4
    // 1,0,2,2  0,1,1,2.  The steps as shifts; an odd pass starts half an x step in, an even pass
    // after the first half a y step down.
    const int lx = interlace ? 3 - (p >> 1) : 0, ly = interlace ? 3 - (p >> 1) + (p > 0 && !(p & 1)) : 0;
    const int xs = (p & 1) ? (1 << lx) >> 1 : 0;
    const int ys = p >= 2 && !(p & 1) ? (1 << ly) >> 1 : 0;
    const int pw = w > xs ? (w - xs + (1 << lx) - 1) >> lx : 0;
    const int ph = h > ys ? (h - ys + (1 << ly) - 1) >> ly : 0;
    const int64_t rb = ((int64_t)pw * bits + 7) >> 3;
    const bool some = pw > 0 && ph > 0;
    if (p == slot) {
      ps->xs = xs;
      ps->ys = ys;
      ps->dx = 1 << lx;
      ps->dy = 1 << ly;
      ps->w = pw;
      ps->h = ph;
      ps->rowbytes = rb;
      ps->off = off;
      return some;
    }
    if (some) off += (int64_t)ph * (1 + rb);
  }
  ps->xs = ps->ys = ps->w = ps->h = 0;
  ps->dx = ps->dy = 1;
  ps->rowbytes = 0;
  ps->off = off;  // slot == number of passes: the exact inflated size
  return false;
}

// The exact inflated size: the sum of the non-empty passes.
SDSJ_HD inline int64_t png_layout_bytes(int w, int h, int ctype, int depth, int interlace) {
  PngPass ps;
  png_pass_at(w, h, ctype, depth, interlace, interlace ? 7 : 1, &ps);
  return ps.off;
}

// The whole layout for host code: the filter unit, the non-empty passes in stream order, the total.
struct PngLayout {
  int32_t unit, npass;
  int64_t total;
  PngPass pass[7];
};

SDSJ_HD inline void png_layout(int w, int h, int ctype, int depth, int interlace, PngLayout* L) {
  L->unit = png_unit(ctype, depth);
  L->npass = 0;
  for (int p = 0; p < (interlace ? 7 : 1); p++)
    if (png_pass_at(w, h, ctype, depth, interlace, p, &L->pass[L->npass])) L->npass++;
  L->total = png_layout_bytes(w, h, ctype, depth, interlace);
}

SDSJ_HD inline uint32_t png_crc_byte(uint32_t c, int b) {  // CRC-32 (reflected 0xEDB88320), one byte, no table
  c ^= (uint32_t)b;
  for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  return c;
}

template <class Reader>
SDSJ_HDI uint32_t png_be32(const Reader& rd, int64_t i) {
  return ((uint32_t)rd(i) << 24) | ((uint32_t)rd(i + 1) << 16) | ((uint32_t)rd(i + 2) << 8) | (uint32_t)rd(i + 3);
}

SDSJ_HD inline uint32_t png_tag(char a, char b, char c, char d) {
  return ((uint32_t)(uint8_t)a << 24) | ((uint32_t)(uint8_t)b << 16) | ((uint32_t)(uint8_t)c << 8) | (uint32_t)(uint8_t)d;
}

template <class Reader>
SDSJ_HD inline bool png_signature(const Reader& rd, int64_t n) {
  return n >= 8 && rd(0) == 0x89 && rd(1) == 'P' && rd(2) == 'N' && rd(3) == 'G' && rd(4) == 0x0D && rd(5) == 0x0A &&
         rd(6) == 0x1A && rd(7) == 0x0A;
}

// ------------------------------------------------------------------------------------------
// iCCP, zTXt and iTXt (SDSJ_FORMAT_PNG_META).  Their handlers in PngImagePlugin.py inflate a zlib stream
// with _safe_zlib_decompress (:145), which raises ValueError only when kPngMaxTextChunk bytes have been
// produced and input is left, and swallow zlib.error; the text chunks add their character counts to a
// budget (check_text_memory :403) that raises above kPngMaxTextMemory.
// ------------------------------------------------------------------------------------------
constexpr int64_t kPngMaxTextChunk = 1 << 20;    // PngImagePlugin.MAX_TEXT_CHUNK
constexpr int64_t kPngMaxTextMemory = 64 << 20;  // PngImagePlugin.MAX_TEXT_MEMORY

template <class Reader>
SDSJ_HDI int64_t png_find_nul(const Reader& rd, int64_t p, int64_t e) {  // the first 0 byte of [p, e), or e
  while (p < e && rd(p) != 0) p++;
  return p;
}

// What the handler of a compressed-metadata chunk with payload [p, e) does.  0: it raises (or this path
// does not know): PIL decides.  1: it accepts without inflating; *text = the bytes that join the text
// budget.  2: it inflates [*zs, e): accepted iff that stream passes the size rule (png_inflate_count), its
// inflated size then joins the budget when *text is 1.  Every byte read lies in [p, e).
//   chunk_iCCP :424  i = s.find(b"\0"), method = s[i + 1] (IndexError when missing, SyntaxError when not
//                    0; without a NUL i = -1 and the method is s[0], which is then not 0), stream s[i+2:]
//   chunk_zTXt :593  split at the first NUL; no NUL or nothing after it: method 0, empty stream, accepted;
//                    otherwise the method must be 0; the text counts when the key is not empty
//   chunk_iTXt :628  early returns (no NUL, fewer than two bytes after it, fewer than two further NULs, a
//                    compressed text with a method other than 0) add nothing; a text's byte length bounds
//                    its character count
template <class Reader>
SDSJ_HDI int png_meta_stream(const Reader& rd, uint32_t tag, int64_t p, int64_t e, int64_t* zs, int64_t* text) {
  *zs = e;
  *text = 0;
  const int64_t i = png_find_nul(rd, p, e);
  if (tag == png_tag('i', 'C', 'C', 'P')) {
    if (i + 1 >= e || rd(i + 1) != 0) return 0;
    *zs = i + 2;
    return 2;
  }
  if (tag == png_tag('z', 'T', 'X', 't')) {
    if (i + 1 >= e) return 1;
    if (rd(i + 1) != 0) return 0;
    *zs = i + 2;
    *text = i > p;
    return 2;
  }
  if (tag != png_tag('i', 'T', 'X', 't')) return 0;
  if (i >= e || e - (i + 1) < 2) return 1;
  const int cf = rd(i + 1), cm = rd(i + 2);
  const int64_t j = png_find_nul(rd, i + 3, e);
  if (j >= e) return 1;
  const int64_t k = png_find_nul(rd, j + 1, e);
  if (k >= e) return 1;
  if (cf == 0) {
    *text = e - (k + 1);
    return 1;
  }
  if (cm != 0) return 1;
  *zs = k + 1;
  *text = 1;
  return 2;
}

// The rule for one chunk that is neither IHDR, PLTE, tRNS, IDAT nor IEND, before the image data and --
// with SDSJ_FORMAT_PNG_META -- after it: its type and length, and for iCCP / zTXt the method byte.  (The
// zlib streams and the text budget are png_meta_chunk's.)  [p, p + len) is the payload, inside the input.
template <class Reader>
SDSJ_HDI bool png_chunk_ok(const Reader& rd, uint32_t tag, int64_t p, uint32_t len, int formats) {
  if (tag == png_tag('g', 'A', 'M', 'A')) return len == 4;
  if (tag == png_tag('c', 'H', 'R', 'M')) return len == 32;
  if (tag == png_tag('s', 'R', 'G', 'B')) return len == 1;
  if (tag == png_tag('p', 'H', 'Y', 's')) return len == 9;
  if (tag == png_tag('t', 'E', 'X', 't')) return len <= 65536;
  if (tag == png_tag('i', 'C', 'C', 'P') || tag == png_tag('z', 'T', 'X', 't') || tag == png_tag('i', 'T', 'X', 't')) {
    int64_t zs, text;
    return (formats & SDSJ_FORMAT_PNG_META) && png_meta_stream(rd, tag, p, p + (int64_t)len, &zs, &text) != 0;
  }
  // acTL (APNG), unknown critical chunks: PIL decides; so it does for eXIf and the ancillary chunks it
  // has no handler for unless the mask has SDSJ_FORMAT_PNG_EXT
  bool letters = true;
  for (int k = 0; k < 4; k++) {
    const int c = (int)((tag >> (8 * k)) & 255u) | 32;
    letters = letters && c >= 'a' && c <= 'z';
  }
  const bool handled = tag == png_tag('a', 'c', 'T', 'L') || tag == png_tag('f', 'c', 'T', 'L') ||
                       tag == png_tag('f', 'd', 'A', 'T') || tag == png_tag('t', 'R', 'N', 'S');  // (tRNS: png_parse's own rule)
  return (formats & SDSJ_FORMAT_PNG_EXT) && letters && ((tag >> 29) & 1u) && !handled;
}

// Signature, IHDR, the chunks before the first IDAT.  Image.open reads exactly these chunks and
// verifies the CRC of each (PngImagePlugin.py ChunkStream.crc), so a mismatch in any of them is an
// error there; a chunk whose handler could raise or that this path has not been checked against
// (acTL, unknown ones, ... and iCCP, zTXt, iTXt without SDSJ_FORMAT_PNG_META) hands the sample over
// instead of guessing.
// h's IHDR fields are filled as soon as IHDR has been read, whatever the status.
//
// formats with SDSJ_FORMAT_PNG_EXT: Adam7 files and every legal (colour type, depth) pair are accepted,
// and so is an ancillary chunk (bit 5 of the first type byte, four ASCII letters -- ChunkStream.read
// raises on a type that is_cid does not match, PngImagePlugin.py:63, :181) that PngStream has no
// chunk_XXXX method for: PngImageFile._open then reads it and checks its CRC like every other
// (:786-792).  The methods of Pillow 12.2.0 are chunk_iCCP :424, IHDR :452, IDAT :473, IEND :486, PLTE
// :490, tRNS :498, gAMA :521, cHRM :528, sRGB :538, pHYs :555, tEXt :573, zTXt :593, iTXt :628, eXIf
// :671, acTL :678, fcTL :699, fdAT :729.  eXIf's only stores the bytes (:671-675) and is accepted too;
// iCCP, zTXt and iTXt inflate data and can raise, the APNG chunks change what is decoded: PIL decides.
//
// formats with SDSJ_FORMAT_PNG_META: iCCP, zTXt and iTXt are accepted here by their structure and CRC
// (png_chunk_ok, png_meta_stream); their zlib streams, the text budget and the chunks after the image data
// are png_meta_check's, which the caller runs on a sample this function accepted (k_png_meta on the
// device, host_png_meta for host planning and the probe).
template <class Reader>
SDSJ_HD int png_parse(const Reader& rd, int64_t n, PngHdr* h, int formats = SDSJ_FORMAT_PNG) {
  const bool ext = (formats & SDSJ_FORMAT_PNG_EXT) != 0;
  h->width = h->height = h->bit_depth = h->ctype = h->interlace = h->bpp = h->plte_n = h->zero = 0;
  h->plte_pos = h->idat_pos = 0;
  if (!png_signature(rd, n)) return SDSJ_UNSUPPORTED;
  int64_t p = 8;
  bool first = true;
  for (;;) {
    if (p + 12 > n) return SDSJ_CORRUPT;  // no room for length, type and CRC
    if (p > kPngMaxHeader) return SDSJ_UNSUPPORTED;
    const uint32_t len = png_be32(rd, p), tag = png_tag((char)rd(p + 4), (char)rd(p + 5), (char)rd(p + 6), (char)rd(p + 7));
    if (first != (tag == png_tag('I', 'H', 'D', 'R'))) return first ? SDSJ_CORRUPT : SDSJ_UNSUPPORTED;
    if (tag == png_tag('I', 'D', 'A', 'T')) {
      h->idat_pos = p;
      break;
    }
    if (len > (uint32_t)kPngMaxHeader || p + 12 + (int64_t)len > n) return SDSJ_CORRUPT;
    if (first) {
      if (len != 13) return SDSJ_CORRUPT;
      h->width = (int32_t)png_be32(rd, p + 8);
      h->height = (int32_t)png_be32(rd, p + 12);
      h->bit_depth = rd(p + 16);
      h->ctype = rd(p + 17);
      h->interlace = rd(p + 20);
    }
    uint32_t crc = 0xFFFFFFFFu;
    for (int64_t i = p + 4; i < p + 8 + (int64_t)len; i++) crc = png_crc_byte(crc, rd(i));
    if ((crc ^ 0xFFFFFFFFu) != png_be32(rd, p + 8 + len)) return SDSJ_CORRUPT;
    if (first) {
      first = false;
      if (h->width <= 0 || h->height <= 0 || rd(p + 18) != 0 || rd(p + 19) != 0 || h->interlace > 1) return SDSJ_CORRUPT;
      const int ct = h->ctype, bd = h->bit_depth;
      const bool pow2 = bd == 1 || bd == 2 || bd == 4 || bd == 8 || bd == 16;
      const bool legal = pow2 && (ct == 0 || (ct == 3 && bd <= 8) || ((ct == 2 || ct == 4 || ct == 6) && bd >= 8));
      if (!legal) return SDSJ_CORRUPT;
      h->bpp = png_unit(ct, bd);
    } else if (tag == png_tag('P', 'L', 'T', 'E')) {
      if (h->plte_n || len == 0 || len > 768 || len % 3) return SDSJ_UNSUPPORTED;
      h->plte_n = (int32_t)(len / 3);
      h->plte_pos = p + 8;
    } else if (tag == png_tag('t', 'R', 'N', 'S')) {  // ignored by convert("RGB"); its handler indexes by colour type
      if (len > 256 || (h->ctype == 0 && len != 2) || (h->ctype == 2 && len != 6)) return SDSJ_UNSUPPORTED;
    } else if (!png_chunk_ok(rd, tag, p + 8, len, formats)) {
      return SDSJ_UNSUPPORTED;
    }
    p += 12 + (int64_t)len;
  }
  if (first) return SDSJ_CORRUPT;
  if (!ext && (h->interlace || h->bit_depth != 8)) return SDSJ_UNSUPPORTED;
  if ((int64_t)h->width * h->height > kPngMaxPixels || h->width > 65535 || h->height > 65535) return SDSJ_UNSUPPORTED;
  const bool plain = h->bit_depth == 8 && !h->interlace;  // one pass of whole-byte pixels: no walk over the passes
  const int64_t raw = plain ? (int64_t)h->height * (1 + (int64_t)h->width * h->bpp)
                            : png_layout_bytes(h->width, h->height, h->ctype, h->bit_depth, h->interlace);
  if (raw > kPngMaxRaw) return SDSJ_UNSUPPORTED;
  return SDSJ_OK;
}

// The inflated size of a non-interlaced image of whole-byte pixels (png_layout_bytes in general).
SDSJ_HD inline int64_t png_raw_bytes(int w, int h, int bpp) { return (int64_t)h * (1 + (int64_t)w * bpp); }

// ------------------------------------------------------------------------------------------
// Bit reader over the IDAT chain (LSB first, RFC 1951).  At the end of a chunk's payload it skips the
// CRC (PIL does not check IDAT CRCs) and reads the next length and type; a type other than IDAT, a
// chunk that leaves the input, or the end of the input end the data.  No byte outside [0, n) is read.
// ------------------------------------------------------------------------------------------
template <class Reader>
struct PngBits {
  Reader rd;  // (by value: a reader with state, such as the device's LDS window, keeps it in registers)
  int64_t n, pos, chunk_end;
  uint64_t buf;
  int32_t cnt;
  int32_t ended;  // no more IDAT data
};

template <class Reader>
SDSJ_HDI bool png_hop(PngBits<Reader>& b) {  // positions on the next IDAT payload byte; false: none
  while (b.pos == b.chunk_end) {
    if (b.ended) return false;
    const int64_t q = b.chunk_end + 4;  // past the CRC
    if (q + 8 > b.n) {
      b.ended = 1;
      return false;
    }
    const uint32_t len = png_be32(b.rd, q), tag = png_be32(b.rd, q + 4);
    if (tag != png_tag('I', 'D', 'A', 'T') || len > 0x7FFFFFFFu || q + 8 + (int64_t)len > b.n) {
      b.ended = 1;
      return false;
    }
    b.pos = q + 8;
    b.chunk_end = b.pos + (int64_t)len;
  }
  return true;
}

template <class Reader>
SDSJ_HDI void png_bits_init(PngBits<Reader>& b, const Reader& rd, int64_t n, int64_t idat_pos) {
  b.rd = rd;
  b.n = n;
  b.buf = 0;
  b.cnt = 0;
  b.ended = 0;
  // idat_pos is the first IDAT's length field: enter it as if a previous chunk's CRC ended 4 bytes before
  b.pos = b.chunk_end = idat_pos - 4;
}

template <class Reader>
SDSJ_HDI void png_fill(PngBits<Reader>& b) {  // as many whole bytes as fit below 57 bits
  if (b.chunk_end - b.pos >= 8 && b.cnt <= 48) {  // inside a chunk: eight independent reads, the bytes that fit are kept
    uint64_t v = 0;
    for (int j = 0; j < 8; j++) v |= (uint64_t)(uint32_t)b.rd(b.pos + j) << (8 * j);
    const int k = (56 - b.cnt) >> 3;  // 1..7 bytes
    v &= (1ull << (8 * k)) - 1;
    b.buf |= v << b.cnt;
    b.pos += k;
    b.cnt += 8 * k;
    return;
  }
  while (b.cnt <= 48) {
    if (b.pos == b.chunk_end && !png_hop(b)) return;
    b.buf |= (uint64_t)(uint32_t)b.rd(b.pos++) << b.cnt;
    b.cnt += 8;
  }
}

template <class Reader>
SDSJ_HDI bool png_take(PngBits<Reader>& b, int k, uint32_t* v) {  // k <= 32 bits, false: data exhausted
  if (b.cnt < k) png_fill(b);
  if (b.cnt < k) return false;
  *v = (uint32_t)(b.buf & ((1ull << k) - 1));
  b.buf >>= k;
  b.cnt -= k;
  return true;
}

// What follows the image data.  PIL's load_end walks the chunks after the last IDAT it consumed and
// calls their handlers, which can raise; this path accepts only what it is sure of: further IDAT
// chunks (skipped there too), then IEND or the end of the input.
template <class Reader>
SDSJ_HDI bool png_tail_ok(PngBits<Reader>& b) {
  for (;;) {
    b.pos = b.chunk_end;
    if (png_hop(b)) continue;
    const int64_t q = b.chunk_end + 4;
    if (q + 8 > b.n) return true;  // the input ends: PIL stops on the short read
    const uint32_t len = png_be32(b.rd, q), tag = png_be32(b.rd, q + 4);
    return tag == png_tag('I', 'E', 'N', 'D') && len == 0;
  }
}

// ------------------------------------------------------------------------------------------
// Deflate tables: canonical counts and sorted symbols (the search for long codes) plus a first-level
// lookup of kInfLut bits: entry = symbol << 4 | code length, 0 = a longer or unused code.
// ------------------------------------------------------------------------------------------
constexpr int kInfLutBits = 9;
constexpr int kInfLut = 1 << kInfLutBits;

struct InfCode {
  uint16_t cnt[16];
  uint16_t lut[kInfLut];
};

struct InfTables {
  InfCode ll, d;
  uint16_t ll_sym[288];
  uint16_t d_sym[32];
  uint8_t lens[320];  // 288 + 32
};

SDSJ_HD inline uint32_t inf_rev(uint32_t code, int len) {
  uint32_t r = 0;
  for (int k = 0; k < len; k++) r |= ((code >> k) & 1u) << (len - 1 - k);
  return r;
}

// zlib inftrees.c inflate_table's checks: an over-subscribed set is an error; an incomplete set is an
// error unless its longest code has one bit (`strict`: the dynamic blocks' literal/length and distance
// sets); a set without any code is accepted, and every code of it is then invalid.
SDSJ_HD inline bool inf_build(const uint8_t* lens, int n, InfCode* c, uint16_t* sym, bool strict) {
  for (int l = 0; l < 16; l++) c->cnt[l] = 0;
  for (int i = 0; i < n; i++) c->cnt[lens[i] & 15]++;
  for (int i = 0; i < kInfLut; i++) c->lut[i] = 0;
  int left = 1, maxl = 0;
  for (int l = 1; l < 16; l++) {
    left <<= 1;
    left -= c->cnt[l];
    if (left < 0) return false;
    if (c->cnt[l]) maxl = l;
  }
  if (maxl == 0) {
    c->cnt[0] = (uint16_t)n;
    return true;
  }
  if (left > 0 && strict && maxl != 1) return false;
  uint16_t offs[16], next[16];
  offs[1] = 0;
  next[0] = 0;
  next[1] = 0;
  uint32_t code = 0;
  for (int l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + c->cnt[l]);
  for (int l = 1; l < 16; l++) {
    code = (code + (l > 1 ? c->cnt[l - 1] : 0)) << (l > 1 ? 1 : 0);
    next[l] = (uint16_t)code;
  }
  for (int i = 0; i < n; i++) {
    const int l = lens[i] & 15;
    if (!l) continue;
    sym[offs[l]++] = (uint16_t)i;
    const uint32_t cd = next[l]++;
    if (l <= kInfLutBits) {
      const uint32_t r = inf_rev(cd, l);
      for (uint32_t k = r; k < (uint32_t)kInfLut; k += 1u << l) c->lut[k] = (uint16_t)((i << 4) | l);
    }
  }
  return true;
}

// One symbol: -1 = invalid code or data exhausted.
template <class Reader>
SDSJ_HDI int inf_decode(PngBits<Reader>& b, const InfCode* c, const uint16_t* sym) {
  if (b.cnt < 15) png_fill(b);
  const uint32_t e = c->lut[b.buf & (kInfLut - 1)];
  if (e) {
    const int l = (int)(e & 15);
    if (l > b.cnt) return -1;
    b.buf >>= l;
    b.cnt -= l;
    return (int)(e >> 4);
  }
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; l++) {
    if (l > b.cnt) return -1;
    code |= (int)((b.buf >> (l - 1)) & 1);
    const int count = c->cnt[l];
    if (code - count < first) {
      b.buf >>= l;
      b.cnt -= l;
      return sym[index + (code - first)];
    }
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

SDSJ_HD inline void inf_fixed_lens(uint8_t* lens) {
  for (int i = 0; i < 144; i++) lens[i] = 8;
  for (int i = 144; i < 256; i++) lens[i] = 9;
  for (int i = 256; i < 280; i++) lens[i] = 7;
  for (int i = 280; i < 288; i++) lens[i] = 8;
  for (int i = 0; i < 32; i++) lens[288 + i] = 5;
}

// Block header.  type 0: *stored = LEN (the reader is byte-aligned on its first byte); 1 / 2: T holds
// the block's tables.  False: an error (type 3, LEN/NLEN mismatch, bad code lengths, data exhausted).
template <class Reader>
SDSJ_HDI bool inf_block_header(PngBits<Reader>& b, InfTables* T, int* final, int* type, int* stored) {
  uint32_t v;
  if (!png_take(b, 3, &v)) return false;
  *final = (int)(v & 1);
  *type = (int)(v >> 1);
  if (*type == 3) return false;
  if (*type == 0) {
    const int drop = b.cnt & 7;  // whole bytes are buffered: the bits up to the byte boundary
    b.buf >>= drop;
    b.cnt -= drop;
    if (!png_take(b, 32, &v)) return false;
    if ((v & 0xFFFFu) != ((v >> 16) ^ 0xFFFFu)) return false;
    *stored = (int)(v & 0xFFFFu);
    return true;
  }
  if (*type == 1) {
    inf_fixed_lens(T->lens);
    return inf_build(T->lens, 288, &T->ll, T->ll_sym, false) && inf_build(T->lens + 288, 32, &T->d, T->d_sym, false);
  }
  if (!png_take(b, 14, &v)) return false;
  const int nlen = (int)(v & 31) + 257, ndist = (int)((v >> 5) & 31) + 1, ncode = (int)(v >> 10) + 4;
  if (nlen > 286 || ndist > 30) return false;
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint8_t cl[19];
  for (int i = 0; i < 19; i++) cl[i] = 0;
  for (int i = 0; i < ncode; i++) {
    if (!png_take(b, 3, &v)) return false;
    cl[order[i]] = (uint8_t)v;
  }
  // the code-length code is decoded with the distance table's storage (rebuilt below)
  if (!inf_build(cl, 19, &T->d, T->d_sym, false)) return false;
  {  // inflate_table(CODES): an incomplete code-length code is an error
    int left = 1;
    for (int l = 1; l < 16; l++) left = (left << 1) - T->d.cnt[l];
    if (left > 0) return false;
  }
  int i = 0;
  while (i < nlen + ndist) {
    const int s = inf_decode(b, &T->d, T->d_sym);
    if (s < 0) return false;
    if (s < 16) {
      T->lens[i++] = (uint8_t)s;
      continue;
    }
    int rep, val = 0;
    if (s == 16) {
      if (i == 0 || !png_take(b, 2, &v)) return false;
      val = T->lens[i - 1];
      rep = 3 + (int)v;
    } else if (s == 17) {
      if (!png_take(b, 3, &v)) return false;
      rep = 3 + (int)v;
    } else {
      if (!png_take(b, 7, &v)) return false;
      rep = 11 + (int)v;
    }
    if (i + rep > nlen + ndist) return false;
    while (rep--) T->lens[i++] = (uint8_t)val;
  }
  if (T->lens[256] == 0) return false;  // no end-of-block code
  // the distance lengths follow the literal/length ones: move them before ll's build reuses nothing of
  // them (separate arrays), then build both sets
  uint8_t dl[32];
  for (int k = 0; k < ndist; k++) dl[k] = T->lens[nlen + k];
  for (int k = 0; k < ndist; k++) T->lens[288 + k] = dl[k];
  return inf_build(T->lens, nlen, &T->ll, T->ll_sym, true) && inf_build(T->lens + 288, ndist, &T->d, T->d_sym, true);
}

// Length / distance of a match from its symbol (base + extra bits).  False: invalid symbol or data exhausted.
template <class Reader>
SDSJ_HDI bool inf_length(PngBits<Reader>& b, int sym, int* len) {
  const uint16_t base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  const uint8_t ext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  const int k = sym - 257;
  if (k < 0 || k >= 29) return false;
  uint32_t v = 0;
  if (ext[k] && !png_take(b, ext[k], &v)) return false;
  *len = base[k] + (int)v;
  return true;
}

template <class Reader>
SDSJ_HDI bool inf_distance(PngBits<Reader>& b, const InfTables* T, int* dist) {
  const uint16_t base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
  const uint8_t ext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
  const int s = inf_decode(b, &T->d, T->d_sym);
  if (s < 0 || s >= 30) return false;
  uint32_t v = 0;
  if (ext[s] && !png_take(b, ext[s], &v)) return false;
  *dist = base[s] + (int)v;
  return true;
}

// A match is valid when its source lies inside the bytes produced so far and inside the window the
// zlib header declares, and its end inside the expected output.
SDSJ_HD inline bool inf_match_ok(int64_t produced, int64_t expect, int dist, int len, int window) {
  return dist >= 1 && (int64_t)dist <= produced && dist <= window && produced + len <= expect;
}

// zlib header (RFC 1950): deflate, window <= 32 KiB, check bits, no preset dictionary.
template <class Reader>
SDSJ_HDI bool zlib_header(PngBits<Reader>& b, int* window) {
  uint32_t v;
  if (!png_take(b, 16, &v)) return false;
  const uint32_t cmf = v & 0xFF, flg = v >> 8;
  if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 || (flg & 0x20)) return false;
  *window = 1 << ((cmf >> 4) + 8);
  return true;
}

// The whole stream into `out` (see the sinks of sdsj_png.hip and tests/asan/png_driver.cpp):
//   out.lit(byte)          appends one byte
//   out.match(dist, len)   appends len bytes copied from dist bytes back (overlap allowed)
// The sink never sees a byte beyond `expect` or a source before the first byte: both end the image
// here.  Returns SDSJ_OK when the stream is well formed, ends in a final block and produced exactly
// `expect` bytes; *adler = the trailer's value (the caller compares it with the output's).  SDSJ_UNSUPPORTED
// is png_tail_ok's answer alone, *adler being set: a caller for whom png_meta_check has judged what follows
// the image data takes it for SDSJ_OK (k_png_inflate_meta).
template <class Reader, class Sink>
SDSJ_HDI int png_inflate(PngBits<Reader>& b, InfTables* T, Sink& out, int64_t expect, uint32_t* adler) {
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
  if (!png_tail_ok(b)) return SDSJ_UNSUPPORTED;
  return SDSJ_OK;
}

// ------------------------------------------------------------------------------------------
// SDSJ_FORMAT_PNG_META: the size rule, the text budget and the chunks after the image data.
// ------------------------------------------------------------------------------------------
// A bit reader confined to one chunk's payload [p, e): no hop to a next chunk.
template <class Reader>
SDSJ_HDI void png_bits_span(PngBits<Reader>& b, const Reader& rd, int64_t n, int64_t p, int64_t e) {
  b.rd = rd;
  b.n = n;
  b.buf = 0;
  b.cnt = 0;
  b.ended = 1;
  b.pos = p;
  b.chunk_end = e;
}

// The size rule: the zlib stream inflated without output or window.  True iff it is well formed up to the
// end of a final block and produces fewer than kPngMaxTextChunk bytes (*count).  zlib then produces no
// more than that either -- it decodes the same symbols, and stops earlier where it also checks what is
// not checked here (match distances, the Adler-32) -- so _safe_zlib_decompress cannot raise.  Everything
// else is refused, including the malformed streams whose zlib.error PIL swallows.
template <class Reader>
SDSJ_HDI bool png_inflate_count(PngBits<Reader>& b, InfTables* T, int64_t* count) {
  int window = 0;
  if (!zlib_header(b, &window)) return false;
  int64_t produced = 0;
  for (;;) {
    int final = 0, type = 0, stored = 0;
    if (!inf_block_header(b, T, &final, &type, &stored)) return false;
    if (type == 0) {
      produced += stored;
      // the buffered whole bytes first, the rest by position (the reader is confined to its payload)
      const int have = b.cnt >> 3, drop = stored < have ? stored : have;
      b.buf = drop < 8 ? b.buf >> (8 * drop) : 0;
      b.cnt -= 8 * drop;
      const int64_t rest = stored - drop;
      if (rest > b.chunk_end - b.pos) return false;
      b.pos += rest;
    } else {
      for (;;) {
        const int s = inf_decode(b, &T->ll, T->ll_sym);
        if (s < 0) return false;
        if (s == 256) break;
        int len = 1, dist = 0;
        if (s > 256 && (!inf_length(b, s, &len) || !inf_distance(b, T, &dist))) return false;
        produced += len;
        if (produced >= kPngMaxTextChunk) return false;
      }
    }
    if (produced >= kPngMaxTextChunk) return false;
    if (final) break;
  }
  *count = produced;
  return true;
}

// One chunk png_chunk_ok accepted, payload [p, p + len) inside the input: its share of the text budget
// (tEXt: its payload, an upper bound of the value's length) and, for iCCP / zTXt / iTXt, the size rule.
template <class Reader>
SDSJ_HDI bool png_meta_chunk(Reader& rd, int64_t n, uint32_t tag, int64_t p, uint32_t len, InfTables* T, int64_t* budget) {
  if (tag == png_tag('t', 'E', 'X', 't')) {
    *budget += (int64_t)len;
  } else if (tag == png_tag('i', 'C', 'C', 'P') || tag == png_tag('z', 'T', 'X', 't') || tag == png_tag('i', 'T', 'X', 't')) {
    int64_t zs = 0, text = 0;
    const int kind = png_meta_stream(rd, tag, p, p + (int64_t)len, &zs, &text);
    if (kind == 0) return false;
    if (kind == 1) {
      *budget += text;
    } else {
      PngBits<Reader> b;
      png_bits_span(b, rd, n, zs, p + (int64_t)len);
      int64_t count = 0;
      const bool ok = png_inflate_count(b, T, &count);
      rd = b.rd;  // (a reader with state, the device's LDS window: the copy has moved it)
      if (!ok) return false;
      if (text) *budget += count;
    }
  }
  return *budget <= kPngMaxTextMemory;
}

// With SDSJ_FORMAT_PNG_META, after png_parse accepted the sample (idat_pos: its first IDAT): the size rule
// and the text budget over the chunks before the image data, then the chunks after it as load_end
// (PngImagePlugin.py:1024) walks them -- no CRC is checked there -- under the rule of the same mask
// (png_chunk_ok) and the same budget.  The image data ends with the run of IDAT chunks (PIL skips those the
// zlib stream did not need); the walk ends at IEND or where no chunk header is left after a CRC.  PLTE, tRNS,
// IHDR, an IDAT after another chunk, the APNG chunks, critical and non-letter types, a payload that leaves
// the input and a tail longer than kPngMaxHeader stay with PIL.  SDSJ_OK or SDSJ_UNSUPPORTED; no byte
// outside [0, n) is read.
template <class Reader>
SDSJ_HDI int png_meta_check(Reader rd, int64_t n, int64_t idat_pos, int formats, InfTables* T) {
  int64_t budget = 0;
  int64_t p = 8;
  int64_t tail0 = -1;  // the first chunk after the IDAT run
  for (;;) {
    if (p + 8 > n) return SDSJ_OK;  // the input ends: PIL stops on the short read
    const uint32_t len = png_be32(rd, p), tag = png_be32(rd, p + 4);
    const int64_t e = p + 8 + (int64_t)len;
    if (p >= idat_pos) {  // (before it png_parse has applied png_chunk_ok, and every chunk lies inside the input)
      if (tag == png_tag('I', 'E', 'N', 'D')) return len == 0 ? SDSJ_OK : SDSJ_UNSUPPORTED;
      if (tail0 < 0 && tag == png_tag('I', 'D', 'A', 'T')) {
        if (len > 0x7FFFFFFFu || e > n) return SDSJ_UNSUPPORTED;
        p = e + 4;
        continue;
      }
      if (tail0 < 0) tail0 = p;
      if (p - tail0 > kPngMaxHeader || len > (uint32_t)kPngMaxHeader || e > n) return SDSJ_UNSUPPORTED;
      if (!png_chunk_ok(rd, tag, p + 8, len, formats)) return SDSJ_UNSUPPORTED;
    }
    if (!png_meta_chunk(rd, n, tag, p + 8, len, T, &budget)) return SDSJ_UNSUPPORTED;
    p = e + 4;
  }
}

constexpr uint32_t kAdlerMod = 65521;

// ------------------------------------------------------------------------------------------
// Filters (PNG specification 9.2; ZipDecode.c).  Pixels travel as packed little-endian dwords of bpp
// bytes: raw = the filtered bytes, a = left, b = up, c = up-left (zeros outside the image).
// ------------------------------------------------------------------------------------------
SDSJ_HD inline int png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

SDSJ_HD inline uint32_t png_recon(int ft, uint32_t raw, uint32_t a, uint32_t b, uint32_t c, int bpp) {
  uint32_t r = 0;
  for (int k = 0; k < bpp; k++) {
    const int sh = 8 * k;
    const int x = (int)((raw >> sh) & 255), pa = (int)((a >> sh) & 255), pb = (int)((b >> sh) & 255),
              pc = (int)((c >> sh) & 255);
    const int pred = ft == 0 ? 0 : ft == 1 ? pa : ft == 2 ? pb : ft == 3 ? ((pa + pb) >> 1) : png_paeth(pa, pb, pc);
    r |= (uint32_t)((x + pred) & 255) << sh;
  }
  return r;
}

// The same over a filter unit of up to 8 bytes (16-bit samples: 2, 4, 6 or 8 bytes a pixel), byte k of
// the unit at bits 8k.
SDSJ_HD inline uint64_t png_recon(int ft, uint64_t raw, uint64_t a, uint64_t b, uint64_t c, int unit) {
  const uint32_t lo = png_recon(ft, (uint32_t)raw, (uint32_t)a, (uint32_t)b, (uint32_t)c, unit < 4 ? unit : 4);
  const uint32_t hi = unit > 4 ? png_recon(ft, (uint32_t)(raw >> 32), (uint32_t)(a >> 32), (uint32_t)(b >> 32),
                                           (uint32_t)(c >> 32), unit - 4)
                               : 0u;
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// The reconstructed pixel as convert("RGB") gives it: gray replicated, alpha dropped (no
// premultiplication), palette entries looked up -- (0, 0, 0) at or beyond the PLTE length or without
// a PLTE.  `pal(i)` returns palette byte i (3 per entry).  Returns r | g << 8 | b << 16.
template <class Pal>
SDSJ_HD inline uint32_t png_rgb(int ctype, uint32_t px, int plte_n, const Pal& pal) {
  const uint32_t v = px & 255;
  switch (ctype) {
    case 0:
    case 4:
      return v | (v << 8) | (v << 16);
    case 3:
      if ((int)v >= plte_n) return 0;
      return (uint32_t)pal(3 * (int)v) | ((uint32_t)pal(3 * (int)v + 1) << 8) | ((uint32_t)pal(3 * (int)v + 2) << 16);
    default:
      return px & 0xFFFFFFu;
  }
}

// Pixel k of a reconstructed filter unit at any depth, as convert("RGB") gives it.  Depths 1, 2, 4: the
// unit is one byte of 8 / 4 / 2 samples, most significant bits first (the caller drops those beyond
// the row's width); gray samples scale by 255 / 85 / 17, palette indices are looked up as png_rgb does.
// Depth 16, samples big-endian: gray alone opens as I;16 and convert("RGB") clips the value to 255;
// gray + alpha, RGB and RGBA keep the high byte of each colour sample.  k is 0 from depth 8 on.
template <class Pal>
SDSJ_HD inline uint32_t png_rgb_ext(int ctype, int depth, uint64_t unit, int k, int plte_n, const Pal& pal) {
  if (depth == 8) return png_rgb(ctype, (uint32_t)unit, plte_n, pal);
  if (depth < 8) {
    const uint32_t mask = (1u << depth) - 1u;
    const uint32_t v = ((uint32_t)unit >> (8 - depth * (k + 1))) & mask;
    return png_rgb(ctype, ctype == 3 ? v : v * (255u / mask), plte_n, pal);
  }
  const uint32_t b0 = (uint32_t)unit & 255u, b1 = (uint32_t)(unit >> 8) & 255u;
  if (ctype == 0) {
    const uint32_t v = b0 ? 255u : b1;  // min((b0 << 8) | b1, 255)
    return v | (v << 8) | (v << 16);
  }
  if (ctype == 4) return b0 | (b0 << 8) | (b0 << 16);
  return b0 | ((uint32_t)(unit >> 16) & 255u) << 8 | ((uint32_t)(unit >> 32) & 255u) << 16;
}

// The descriptor of a parsed PNG: no components, blocks or entropy data, so every JPEG kernel that
// walks all images of a batch finds nothing to do for it (they also test `png`).
SDSJ_HD inline void png_fill_desc(ImgDesc* d, const PngHdr& h) {
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
  d->png = 1;
  d->png_ctype = h.ctype;
  d->png_bpp = h.bpp;
  d->png_plte_n = h.plte_n;
  d->png_plte_pos = h.plte_pos;
  d->png_idat_pos = h.idat_pos;
  // (a header png_parse refused may hold any sizes: nothing reads png_raw then)
  if (h.bit_depth == 8 && !h.interlace) d->png_raw = png_raw_bytes(h.width, h.height, h.bpp);
  else d->png_raw = h.width <= 65535 && h.height <= 65535 ? png_layout_bytes(h.width, h.height, h.ctype, h.bit_depth, h.interlace) : 0;
  d->png_depth_lace = (h.bit_depth & 255) | ((h.interlace & 255) << 8);  // (the struct's size and offsets are pinned)
  d->off_png = 0;
}

}  // namespace sdsj
