// sdsj_scan_wave.h -- the wavefront-level pieces the scan-walking JPEG kernels share: k_prog (sdsj_progressive.hip,
// SOF2) and k_scans (sdsj_scans.hip, multi-scan sequential under SDSJ_FORMAT_JPEG_SCANS).  One wave walks an
// image's scans with its decoder state wave-uniform: the bit reader over the stuffed stream with jdhuff.c's
// marker, restart and resynchronisation rules, the derived Huffman tables (jpeg_make_d_derived_tbl) and the
// DHT / DQT bodies read between scans.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdsj_common.h"

namespace sdsj {

namespace {

// Bit reader over the stuffed stream (jdhuff.c jpeg_fill_bit_buffer semantics): FF00 -> FF, FF fill
// bytes skipped; a marker stops the data (zeros are fed from there); the input ending first is eof.
struct PBits {
  const uint8_t* d;
  int n, pos;  // (32-bit: the scans' data is far below 2 GB; fewer scalar registers)
  uint64_t buf;
  int nbits, hit_marker, marker, pad_bits, insufficient, eof;
  uintptr_t wbase;  // 16-byte window of the stream held in registers (one load per 16 bytes)
  uint4 w;
};

// The aligned 16 bytes around p (address a).  Addressed from p itself, not from the integer a: a
// pointer rebuilt from an integer is a flat pointer, whose loads the compiler must treat as
// per-lane values -- the whole bit reader then runs on vector registers under exec masks.  From
// the global pointer the window, and everything decoded from it, is wave-uniform.
__device__ __forceinline__ uint4 pwindow(const uint8_t* p, uintptr_t a) {
  return *reinterpret_cast<const uint4*>(p - (a & 15));
}

// Byte i of the stream (0 <= i < n) through the window: the aligned 16 bytes around it come in as
// one load (the blob allocation holds the whole granule).
__device__ __forceinline__ int pbyte(PBits& b, int i) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(b.d + i), base = a & ~(uintptr_t)15;
  if (base != b.wbase) {
    b.wbase = base;
    b.w = pwindow(b.d + i, a);
  }
  // (the window is picked from computed values, not from field loads: a select between loads of
  // b.w's fields becomes a select between their addresses, and the bit reader state then stays in
  // scratch memory instead of registers)
  const uint32_t o = (uint32_t)(a - base);
  const uint64_t lo = ((uint64_t)b.w.y << 32) | b.w.x, hi = ((uint64_t)b.w.w << 32) | b.w.z;
  return (int)((((o & 8) ? hi : lo) >> (8 * (o & 7))) & 0xFF);
}

__device__ __forceinline__ void pfill(PBits& b) {
  while (b.nbits <= 56) {
    // fast path: 4 bytes inside the window with no 0xFF among them go in at once
    if (b.nbits <= 32 && !b.hit_marker && b.pos + 4 <= b.n) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(b.d + b.pos), base = a & ~(uintptr_t)15;
      const uint32_t o = (uint32_t)(a - base);
      if (o <= 12) {
        if (base != b.wbase) {
          b.wbase = base;
          b.w = pwindow(b.d + b.pos, a);
        }
        // bytes o .. o + 3 of the 16-byte window (a 128-bit shift; see pbyte)
        const uint64_t lo = ((uint64_t)b.w.y << 32) | b.w.x, hi = ((uint64_t)b.w.w << 32) | b.w.z;
        const uint32_t sh = 8 * (o & 7);
        const uint64_t q = (o & 8) ? hi >> sh : (sh ? (lo >> sh) | (hi << (64 - sh)) : lo);
        const uint32_t x = (uint32_t)q, t = ~x;
        if (((t - 0x01010101u) & ~t & 0x80808080u) == 0) {
          b.buf |= (uint64_t)__builtin_bswap32(x) << (32 - b.nbits);
          b.nbits += 32;
          b.pos += 4;
          continue;
        }
      }
    }
    int c;
    if (b.hit_marker || b.pos >= b.n) {
      if (!b.hit_marker) b.eof = 1;
      c = 0;
      b.pad_bits += 8;
    } else {
      c = pbyte(b, b.pos++);
      if (c == 0xFF) {
        int c2;
        do {
          c2 = b.pos < b.n ? pbyte(b, b.pos++) : -1;
        } while (c2 == 0xFF);
        if (c2 == 0) {
          c = 0xFF;
        } else if (c2 < 0) {
          b.pos = b.n;
          continue;
        } else {
          b.hit_marker = 1;
          b.marker = c2;
          b.pos -= 2;  // the marker stays for process_restart / read_markers
          continue;
        }
      }
    }
    b.buf |= (uint64_t)c << (56 - b.nbits);
    b.nbits += 8;
  }
}

// n (1..32) bits the caller knows are in the buffer (phuff left >= 32 after its symbol's start)
__device__ __forceinline__ int pgetbits_nc(PBits& b, int n) {
  const int v = (int)(b.buf >> (64 - n));
  b.buf <<= n;
  b.nbits -= n;
  if (b.nbits < b.pad_bits) b.insufficient = 1;
  return v;
}

__device__ __forceinline__ int pgetbits(PBits& b, int n) {
  if (n == 0) return 0;
  if (b.nbits < n) pfill(b);
  const int v = (int)(b.buf >> (64 - n));
  b.buf <<= n;
  b.nbits -= n;
  if (b.nbits < b.pad_bits) b.insufficient = 1;  // consumed inserted zeros (JWRN_HIT_MARKER)
  return v;
}

// The lookahead tables of the scan being decoded, in LDS (one slot per lane = per image); the
// canonical bounds and symbols that codes of more than 9 bits need stay in ProgTables (global
// memory: such codes are rare, and 4.3 KB of LDS per image instead of 7.4 KB lets more images run
// per CU).
struct PLds {
  uint16_t look[4][1 << 9];  // per scan position: (length << 8) | symbol of the codes of <= 9 bits, 0 = longer
  int32_t qh[4], qv[4], qbo[4], qdsl[4], ldc[4];  // interleaved DC scans: per scan position h, v, block
                                                  // offset in the MCU, DC table slot, DC predictor
  int32_t ins_m;  // the MCU in which the scan ran out of data (-1: none); in LDS, off the MCU loop's registers
};

// jdhuff.c jpeg_huff_decode: codes of <= 9 bits come from the scan position's lookahead table in one
// LDS read; longer (and bad) codes take the first l whose l-bit prefix is <= maxcode[l] (all 16
// compares issue together on 17 peeked bits); no match = bad code: 17 bits, symbol 0.  Bits are
// consumed only after the length is known, so insufficient_data follows the consumed count as with
// a bit-serial decode.
// The buffer holds >= 32 bits when the symbol starts, so its extra bits (<= 15, or 1 + a correction
// bit) need no second check.
__device__ __forceinline__ int phuff(PBits& b, const PLds& L, const ProgTables* __restrict__ T, int slot, int q) {
  if (b.nbits < 32) pfill(b);
  const uint32_t e = L.look[q][(uint32_t)(b.buf >> 55)];
  if (e) {
    const int l = (int)(e >> 8);
    b.buf <<= l;
    b.nbits -= l;
    if (b.nbits < b.pad_bits) b.insufficient = 1;
    return (int)(e & 0xFF);
  }
  const uint32_t peek = (uint32_t)(b.buf >> 47);
  int l = 17;
#pragma unroll
  for (int k = 16; k >= 10; k--) l = (int32_t)(peek >> (17 - k)) <= T->maxcode[slot][k] ? k : l;
  b.buf <<= l;
  b.nbits -= l;
  if (b.nbits < b.pad_bits) b.insufficient = 1;
  if (l > 16) return 0;
  return T->vals[slot][((int32_t)(peek >> (17 - l)) + T->valoff[slot][l]) & 0xFF];
}

__device__ __forceinline__ int pextend(int x, int s) { return x < (1 << (s - 1)) ? x + (int)((~0u << s) + 1) : x; }

// jdmarker.c next_marker from the byte cursor: pos ends on the marker's last FF; -1 at the end
__device__ __forceinline__ int pnext_marker(PBits& b) {
  for (;;) {
    while (b.pos < b.n && pbyte(b, b.pos) != 0xFF) b.pos++;
    if (b.pos >= b.n) return -1;
    int p = b.pos + 1;
    while (p < b.n && pbyte(b, p) == 0xFF) p++;
    if (p >= b.n) return -1;
    const int m = pbyte(b, p);
    if (m != 0) {
      b.pos = p - 1;
      return m;
    }
    b.pos = p + 1;
  }
}

__device__ __forceinline__ void pconsume_marker(PBits& b) {
  b.pos += 2;
  b.hit_marker = 0;
  b.marker = 0;
}

// read_restart_marker + jpeg_resync_to_restart (actions 1 / 2 / 3); -1 when the input ends first
__device__ __forceinline__ int pread_restart(PBits& b, int desired) {
  if (!b.hit_marker) {
    const int m = pnext_marker(b);
    if (m < 0) return -1;
    b.hit_marker = 1;
    b.marker = m;
  }
  if (b.marker == 0xD0 + desired) {
    pconsume_marker(b);
    return 0;
  }
  for (;;) {
    const int m = b.marker;
    int action;
    if (m < 0xC0) action = 2;
    else if (m < 0xD0 || m > 0xD7) action = 3;
    else if (m == 0xD0 + ((desired + 1) & 7) || m == 0xD0 + ((desired + 2) & 7)) action = 3;
    else if (m == 0xD0 + ((desired - 1) & 7) || m == 0xD0 + ((desired - 2) & 7)) action = 2;
    else action = 1;
    if (action == 1) {
      pconsume_marker(b);
      return 0;
    }
    if (action == 3) return 0;
    pconsume_marker(b);
    const int m2 = pnext_marker(b);
    if (m2 < 0) return -1;
    b.hit_marker = 1;
    b.marker = m2;
  }
}

__device__ __forceinline__ int pprocess_restart(PBits& b, int* next_num) {
  b.buf = 0;
  b.nbits = 0;
  b.pad_bits = 0;
  if (pread_restart(b, *next_num)) return -1;
  *next_num = (*next_num + 1) & 7;
  if (!b.hit_marker) b.insufficient = 0;
  return 0;
}

__device__ __forceinline__ int rd16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// jdhuff.c jpeg_make_d_derived_tbl for slot (0..3 DC, 4..7 AC) and scan position q: canonical
// bounds plus the 9-bit lookahead table (entry x: the code of length l <= 9 that is x's l-bit
// prefix, found like jpeg_huff_decode's search; the lanes fill 8 entries each); false when the code
// assignment overflows (JERR_BAD_HUFF_TABLE), or a DC table holds a symbol > 15
__device__ __forceinline__ bool pderive(ProgTables* P, PLds& L, int slot, int q, int lane) {
  if (!P->defined[slot]) return false;
  int code = 0, p = 0;
  int mc[10], vo[10];
#pragma unroll
  for (int l = 1; l <= 16; l++) {
    const int cnt = P->bits[slot][l];
    const int m = cnt ? code + cnt - 1 : -1, o = cnt ? p - code : 0;
    P->maxcode[slot][l] = m;
    P->valoff[slot][l] = o;
    if (l <= 9) {
      mc[l] = m;
      vo[l] = o;
    }
    p += cnt;
    code += cnt;
    if (cnt && code >= (1 << l)) return false;  // (the all-ones code is reserved)
    code <<= 1;
  }
  if (p > 256) return false;
  if (slot < 4)
    for (int i = 0; i < p; i++)
      if (P->vals[slot][i] > 15) return false;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int x = lane + 64 * k;
    int ls = 0, vi = 0;  // (selects, no branches: one symbol load per entry)
#pragma unroll
    for (int l = 9; l >= 1; l--) {
      const int c = x >> (9 - l);
      const bool hit = c <= mc[l];
      ls = hit ? l : ls;
      vi = hit ? c + vo[l] : vi;
    }
    const int sym = P->vals[slot][vi & 0xFF];
    L.look[q][x] = (uint16_t)(ls ? (ls << 8) | sym : 0);
  }
  return true;
}

// get_dht / get_dqt bodies
__device__ __forceinline__ int pread_dht(ProgTables* P, const uint8_t* s, int sl) {
  int k = 0;
  while (k < sl) {
    if (k + 17 > sl) return SDSJ_CORRUPT;
    const int tc = s[k] >> 4, th = s[k] & 15;
    if (tc > 1 || th > 3) return SDSJ_CORRUPT;
    const int slot = tc * 4 + th;
    int cnt = 0;
    P->bits[slot][0] = 0;
    for (int l = 1; l <= 16; l++) {
      P->bits[slot][l] = s[k + l];
      cnt += s[k + l];
    }
    if (cnt > 256 || k + 17 + cnt > sl) return SDSJ_CORRUPT;
    for (int i = 0; i < 256; i++) P->vals[slot][i] = i < cnt ? s[k + 17 + i] : 0;
    P->defined[slot] = 1;
    k += 17 + cnt;
  }
  return SDSJ_OK;
}

__device__ __forceinline__ int pread_dqt(ProgTables* P, const uint8_t* s, int sl) {
  int k = 0;
  while (k < sl) {
    const int pq = s[k] >> 4, tq = s[k] & 15;
    if (tq > 3 || pq > 1) return SDSJ_CORRUPT;
    const int need = 1 + 64 * (pq ? 2 : 1);
    if (k + need > sl) return SDSJ_CORRUPT;
    for (int q = 0; q < 64; q++)
      P->qt[tq][natural_order(q)] = (uint16_t)(pq ? rd16(s + k + 1 + 2 * q) : s[k + 1 + q]);
    P->qt_defined[tq] = 1;
    k += need;
  }
  return SDSJ_OK;
}

// Blocks are kept in zigzag order (the order k_idct reads): zigzag index k is natural_order(k), and
// natural_order's guard entries past 63 are all 63.
__device__ __forceinline__ int zig(int k) { return k < 63 ? k : 63; }

}  // namespace

}  // namespace sdsj
