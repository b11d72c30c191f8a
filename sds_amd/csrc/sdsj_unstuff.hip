// sdsj_unstuff.hip -- gfx950 (MI355X) kernels that unstuff the entropy-coded data of baseline images.
//
// Stage map (reference behaviour each kernel reproduces, see DESIGN.md for the layout/rooflines):
//   k_unstuff  byte unstuffing + RSTn split        jdhuff.c jpeg_fill_bit_buffer / process_restart
//   k_scanmap  restart intervals -> data segments   jdhuff.c process_restart / jdmarker.c read_markers
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdsj_common.h"
#include "sdsj_kernels.h"

#pragma clang fp contract(off)

namespace sdsj {

// ------------------------------------------------------------------------------------------
// Unstuffing: removes FF00 stuffing and fill bytes, splits at RSTn markers and stops at the first
// other marker (jdhuff.c jpeg_fill_bit_buffer semantics).  The entropy-coded data is cut into 8 KiB
// tiles; each thread classifies 32 consecutive bytes (read as realigned dwords).  Three passes over
// the tiles of all images at once:
//   k_us_count  per tile: bytes emitted and split markers before the tile's end marker
//   k_us_scan   per image: exclusive prefixes over its tiles, the tile the scan ends in, lengths
//   k_us_write  per tile: one packed (emitted, split) scan places the bytes, the tile is assembled
//               in LDS and leaves as aligned 16-byte stores (byte stores for the two boundary chunks
//               it shares with its neighbours)
// ------------------------------------------------------------------------------------------
constexpr int kUnstuffThreads = 256;
constexpr int kUsBytes = 32;
constexpr int kUsTile = kUnstuffThreads * kUsBytes;
static_assert(kUsTile == kUsTileBytes, "tile table granularity");
constexpr int kUsGrid = 16;  // virtual workgroups per kRtUsBig image in k_us_count / k_us_write
constexpr int kUsLaunch = 1024;  // workgroups of the route-striding unstuff kernels
constexpr int kUsNone = 0x7fffffff;
constexpr int kUsSkip = 2, kUsFinal = 1;  // UsTile.code after k_us_scan

__device__ __forceinline__ int wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int a = __shfl_up(v, o, 64);
    v += lane >= o ? a : 0;
  }
  return v;
}

// jdmarker.c read_markers after the scan, up to EOI, from the marker whose last FF is raw[pos]
// (thread-serial; normally one step: EOI).
__device__ int post_scan_markers(const uint8_t* raw, int64_t n, int64_t pos) {
  for (int guard = 0; guard < 4096; guard++) {
    if (pos + 1 >= n) return SDSJ_OK;
    const int m = raw[pos + 1];
    const int64_t body = pos + 2;
    if (m == 0xD9) return SDSJ_OK;
    if ((m >= 0xD0 && m <= 0xD7) || m == 0x01) {
      pos = body;
    } else {
      const bool is_seg = (m >= 0xE0 && m <= 0xEF) || m == 0xFE || m == 0xDC || m == 0xCC || m == 0xDD || m == 0xC4 ||
                          m == 0xDB;
      if (!is_seg) return SDSJ_CORRUPT;  // second SOI/SOF/SOS, JPGn, unknown (JERR_*)
      if (body + 2 > n) return SDSJ_OK;
      const int64_t len = (raw[body] << 8) | raw[body + 1];
      if (len < 2) return SDSJ_CORRUPT;
      if (body + len > n) return SDSJ_OK;
      const uint8_t* q = raw + body + 2;
      const int64_t sl = len - 2;
      if (m == 0xDD && len != 4) return SDSJ_CORRUPT;
      if (m == 0xC4) {
        for (int64_t k = 0; k < sl;) {
          if (k + 17 > sl || (q[k] >> 4) > 1 || (q[k] & 15) > 3) return SDSJ_CORRUPT;
          int64_t cnt = 0;
          for (int l = 1; l <= 16; l++) cnt += q[k + l];
          if (cnt > 256 || k + 17 + cnt > sl) return SDSJ_CORRUPT;
          k += 17 + cnt;
        }
      }
      if (m == 0xDB) {
        for (int64_t k = 0; k < sl;) {
          if ((q[k] & 15) > 3) return SDSJ_CORRUPT;
          const int64_t need = 1 + 64 * ((q[k] >> 4) ? 2 : 1);
          if (k + need > sl) return SDSJ_CORRUPT;
          k += need;
        }
      }
      pos = body + len;
    }
    // next_marker: skip data bytes, fill bytes and FF00 pairs
    for (;;) {
      while (pos < n && raw[pos] != 0xFF) pos++;
      if (pos >= n) return SDSJ_OK;
      int64_t p = pos + 1;
      while (p < n && raw[p] == 0xFF) p++;
      if (p >= n) return SDSJ_OK;
      if (raw[p] != 0) {
        pos = p - 1;
        break;
      }
      pos = p + 1;
    }
  }
  return SDSJ_CORRUPT;
}

// Restart intervals -> data segments, then the markers after the scan (one thread; kept out of line
// so its registers do not weigh on the tile loop).
__device__ void finish_scan(ImgDesc* d, const SegView sv, const uint8_t* raw, int64_t L, int m, int end_code,
                                       int64_t end_raw, int64_t out_pos, int overflow) {
  const int nseg = d->nseg;
  int status = SDSJ_OK;
  if (overflow) status = SDSJ_CORRUPT;
  // the input ended inside the scan (no marker): Pillow reports "image file is truncated"
  if (end_code < 0) status = SDSJ_CORRUPT;
  // Restart intervals -> data segments D_0 = [0, mk_out[0]), D_i = [mk_out[i-1], mk_out[i]),
  // D_m = [mk_out[m-1], out_pos); the marker after D_i is mk[i] (i < m) or the end marker.
  // jdhuff.c process_restart -> jdmarker.c read_restart_marker / jpeg_resync_to_restart.
  auto d_lo = [&](int i) { return i == 0 ? 0 : sv.mk_out[i - 1]; };
  auto d_hi = [&](int i) { return i < m ? sv.mk_out[i] : (int32_t)out_pos; };
  int cand = 0;  // the data segment being read / the marker after it
  sv.lo[0] = 0;
  sv.hi[0] = d_hi(0);
  sv.flag[0] = 0;
  for (int k = 1; k < nseg && status == SDSJ_OK; k++) {
    const int desired = (k - 1) & 7;
    for (;;) {
      const int mc = cand < m ? sv.mk_code[cand] : end_code;
      int action;
      if (mc == 0xD0 + desired) action = 1;
      else if (mc < 0xC0) action = 2;
      else if (mc < 0xD0 || mc > 0xD7) action = 3;
      else if (mc == 0xD0 + ((desired + 1) & 7) || mc == 0xD0 + ((desired + 2) & 7)) action = 3;
      else if (mc == 0xD0 + ((desired - 1) & 7) || mc == 0xD0 + ((desired - 2) & 7)) action = 2;
      else action = 1;
      if (action == 1) {  // marker consumed: the interval decodes the next data segment
        cand++;
        sv.lo[k] = d_lo(cand);
        sv.hi[k] = d_hi(cand);
        sv.flag[k] = 0;
        break;
      }
      if (action == 3) {  // marker left unread: an empty segment
        sv.lo[k] = sv.hi[k] = d_hi(cand);
        sv.flag[k] = kSegEmpty;
        break;
      }
      if (cand >= m) {  // (unreachable: the end marker is >= SOF0, an end of input failed above)
        status = SDSJ_CORRUPT;
        break;
      }
      cand++;  // action 2: skip to the next marker
    }
  }
  // jpeg_finish_decompress: markers from the one after the last decoded data up to EOI
  for (; status == SDSJ_OK && cand < m; cand++) {
    const int mc = sv.mk_code[cand];
    if (!((mc >= 0xD0 && mc <= 0xD7) || mc == 0x01)) status = SDSJ_CORRUPT;  // unknown marker
  }
  if (status == SDSJ_OK)
    status = post_scan_markers(raw, d->entropy_off + L, d->entropy_off + end_raw);
  sv.lo[nseg] = sv.hi[nseg] = (int32_t)out_pos;
  if (status != SDSJ_OK) d->status = status;
}

// Bytes [my0, my0 + 32) of the entropy-coded data classified as bit masks (bit k = byte k): FF bytes
// are skipped (fill / stuffing prefix); a byte after FF is a stuffed zero (emitted as 0xFF) or a
// marker code; markers split the data (RSTn, and codes below SOF0: the restart logic decides) or end
// it (any other marker, or the end of the input).  u[1..8] hold the 32 bytes, u[0] the 4 before
// (entropy_off >= 4, so they are header bytes of the same image).
struct UsClass {
  uint32_t u[9];
  uint32_t emit, stuffed, split, endm, vmask;
  uint32_t fillstuff;  // stuffed zeros preceded by two or more FF bytes (FF FF .. 00)
};
__device__ __forceinline__ int us_byte(const UsClass& c, int k) {
  uint32_t dw = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) dw = q == (k >> 2) ? c.u[1 + q] : dw;
  return (int)(dw >> (8 * (k & 3))) & 0xFF;
}
// Bytes past the input are never emitted (us_classify's vmask), so their values do not matter; the 4
// bytes before the entropy-coded data are header bytes.
struct UsRaw {
  uint32_t v[10];
};
// The ten dwords holding bytes [my0 - 4, my0 + 32), from four aligned 16-byte loads covering them:
// (e + my0) & 15 is the same for every thread of the image (tiles and threads start at multiples of
// 16), so the ten dwords sit at a wave-uniform offset into the sixteen loaded.  (Ten dword loads at a
// 32-byte lane stride measured 1.5x slower in k_us_count, profiles/r04_ab.txt.)  Chunks past the one
// holding the input's last byte read that one (same page); a chunk before the one holding byte -4
// (only for my0 = 0 and (e & 15) >= 4, and then unused) reads that one, so nothing before the image's
// headers is touched.  Loads go through the global address space as a native vector (HIP's uint4
// struct is loaded as flat, and flat loads also count on lgkmcnt, i.e. on every LDS wait).
typedef uint32_t us_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void us_load(const uint8_t* e, int64_t L, int64_t my0, UsRaw& r) {
  const uintptr_t a = (uintptr_t)(e + my0) & 15;
  const us_u32x4* A = reinterpret_cast<const us_u32x4*>((uintptr_t)(e + my0) - a - 16);
  const us_u32x4* first = reinterpret_cast<const us_u32x4*>(((uintptr_t)e - 4) & ~(uintptr_t)15);
  const us_u32x4* last = reinterpret_cast<const us_u32x4*>(((uintptr_t)(e + L) - 1) & ~(uintptr_t)15);
  uint32_t D[16];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const us_u32x4* p = A + i < first ? first : A + i;
    const us_u32x4 q = *(const __attribute__((address_space(1))) us_u32x4*)(p < last ? p : last);
    D[4 * i] = q.x;
    D[4 * i + 1] = q.y;
    D[4 * i + 2] = q.z;
    D[4 * i + 3] = q.w;
  }
  switch (__builtin_amdgcn_readfirstlane((int)(a >> 2))) {  // (uniform: static register indices)
#define US_CASE(S)                                                       \
  case S:                                                                \
    _Pragma("unroll") for (int k = 0; k < 10; k++) r.v[k] = D[S + 3 + k]; \
    break;
    US_CASE(0)
    US_CASE(1)
    US_CASE(2)
    default:
    US_CASE(3)
#undef US_CASE
  }
}
__device__ __forceinline__ void us_classify(const uint8_t* e, int64_t L, int64_t my0, const UsRaw& r, UsClass& c) {
  const int sh = (int)((uintptr_t)(e + my0) & 3);
#pragma unroll
  for (int k = 0; k < 9; k++) c.u[k] = (uint32_t)((((uint64_t)r.v[k + 1] << 32) | r.v[k]) >> (8 * sh));
  // per byte (SWAR, bit 7 of each byte lane): zero, 0xFF, and "a marker code that splits the data"
  // (RSTn, or below SOF0), then packed to bit masks (bit k = byte k)
  auto pack = [](uint32_t m) { return ((m >> 7) & 1) | ((m >> 14) & 2) | ((m >> 21) & 4) | ((m >> 28) & 8); };
  auto zbytes = [](uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; };
  uint32_t isff = 0, isz = 0, issp = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) {
    const uint32_t x = c.u[1 + q];
    const uint32_t ge_c0 = x & (x << 1) & 0x80808080u;               // top two bits set
    const uint32_t rst = zbytes((x ^ 0xD0D0D0D0u) & 0xF8F8F8F8u);    // 0xD0..0xD7
    isz |= pack(zbytes(x)) << (4 * q);
    isff |= pack(zbytes(~x)) << (4 * q);
    issp |= pack((~ge_c0 & 0x80808080u) | rst) << (4 * q);
  }
  const uint32_t prevff = (isff << 1) | ((my0 > 0 && (c.u[0] >> 24) == 0xFF) ? 1u : 0u);
  const int64_t nvalid = L - my0;
  c.vmask = nvalid >= kUsBytes ? 0xFFFFFFFFu : (nvalid <= 0 ? 0u : ((1u << nvalid) - 1u));
  const uint32_t marker = prevff & ~isz & ~isff & c.vmask;
  c.stuffed = prevff & isz;
  // FF FF .. 00 (fill bytes before a stuffed zero; not valid JPEG, jdhuff.c jpeg_fill_bit_buffer reads it
  // as one FF data byte): libjpeg-turbo's decode_mcu_fast takes the first FF FF for a marker, decodes the
  // rest of that MCU from zero bits into the coefficient blocks, then decode_mcu_slow re-decodes the MCU
  // over them -- coefficients the slow path leaves zero keep the fast path's values.  Streams that hold it
  // are reported SDSJ_CORRUPT (the transforms rerun them on PIL).
  const uint32_t prev2ff = (isff << 2) | ((my0 > 0 && (c.u[0] >> 24) == 0xFF) ? 2u : 0u) |
                           ((my0 > 0 && ((c.u[0] >> 16) & 0xFF) == 0xFF) ? 1u : 0u);
  c.fillstuff = c.stuffed & prev2ff;
  c.emit = ~isff & ~marker & c.vmask;
  c.split = marker & issp;
  c.endm = (marker & ~issp) | ~c.vmask;  // the first byte past the input ends the data as well
}

// Tile end: the first ending byte of the tile (kUsNone: none), from every thread's classification
// (one barrier; wmin is free again after the caller's next barrier).
__device__ __forceinline__ int us_my_end(const UsClass& c, int t) {
  return c.endm ? t * kUsBytes + __builtin_ctz(c.endm) : kUsNone;
}
__device__ __forceinline__ int us_tile_end(int my_end, int t, int* wmin) {
  int m = my_end;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o, 64));
  if ((t & 63) == 0) wmin[t >> 6] = m;
  __syncthreads();
  int r = wmin[0];
#pragma unroll
  for (int q = 1; q < kUnstuffThreads / 64; q++) r = min(r, wmin[q]);
  return r;
}
// The ending marker's code (-1: the end of the input), from the thread that holds it.
__device__ __forceinline__ int us_end_code(const UsClass& c, int t, int tile_end) {
  const int k = tile_end - t * kUsBytes;
  return ((c.vmask >> k) & 1) ? us_byte(c, k) : -1;
}

__device__ __forceinline__ uint32_t us_below(int tile_end, int t) {
  int lim = tile_end - t * kUsBytes;
  lim = lim < 0 ? 0 : (lim > kUsBytes ? kUsBytes : lim);
  return lim >= kUsBytes ? 0xFFFFFFFFu : ((1u << lim) - 1u);
}

// Places one tile's bytes at output offset obase and its split markers from entry sbase: one packed
// (emitted, split) scan, assembly in LDS, aligned 16-byte stores (byte stores for the boundary chunks
// shared with the neighbouring tiles).  The final tile is followed by kUPad zero bytes (the bit reader
// over-reads) to a 16-byte end.  Returns the tile's packed total.  Block-uniform call; buf and wsum are
// free again after the caller's next barrier.
// buf: [16 + kUsTile + kUPad + 16] bytes; the last 16 take the skipped bytes' stores
__device__ int us_place(const UsClass& c, int64_t my0, int t, int tile_end, int64_t obase, int sbase, bool final,
                        uint8_t* out, const SegView& sv, uint8_t* buf, int* wsum) {
  const int lane = t & 63, wv = t >> 6;
  const uint32_t below = us_below(tile_end, t);
  const uint32_t em = c.emit & below, sp = c.split & below;
  const int packed = __popc(em) | (__popc(sp) << 16);
  const int incl = wave_incl_scan(packed);
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int q = 0; q < kUnstuffThreads / 64; q++) {
    before += q < wv ? wsum[q] : 0;
    total += wsum[q];
  }
  const int excl = before + incl - packed;
  const int head = (int)(obase & 15);  // buf[i] is output byte (obase & ~15) + i
  // an emitted byte is itself, or 0xFF for the stuffed 0x00 of an FF00 pair; every byte is stored
  // (branch-free), the skipped ones to a dummy slot past the tile
  constexpr int kDummy = 16 + kUsTile + kUPad;
  int pos = head + (excl & 0xFFFF);
#pragma unroll
  for (int q = 0; q < kUsBytes / 4; q++) {
    const uint32_t sm = (c.stuffed >> (4 * q)) & 0xF;
    const uint32_t wq = c.u[1 + q] | (((sm * 0x00204081u) & 0x01010101u) * 0xFFu);
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int k = 4 * q + b;
      const int bit = (int)((em >> k) & 1);
      buf[bit ? pos : kDummy] = (uint8_t)(wq >> (8 * b));
      pos += bit;
    }
  }
  int m = sbase + (excl >> 16);
  for (uint32_t mk = sp; mk; m++) {  // rare: the split markers, in order
    const int k = __builtin_ctz(mk);
    mk &= mk - 1;
    if (m < sv.cap) {  // (the image is marked corrupt otherwise)
      sv.mk_out[m] = (int32_t)(obase + (excl & 0xFFFF) + __popc(em & ((1u << k) - 1u)));
      sv.mk_raw[m] = (int32_t)(my0 + k - 1);
      sv.mk_code[m] = us_byte(c, k);
    }
  }
  const int len = head + (total & 0xFFFF);
  const int stop = final ? ((len + kUPad + 15) & ~15) : len;
  for (int i = len + t; i < stop; i += kUnstuffThreads) buf[i] = 0;
  __syncthreads();
  uint8_t* dst = out + (obase & ~(int64_t)15);
  const int first_full = (head + 15) >> 4, end_full = stop >> 4;
  for (int i = first_full + t; i < end_full; i += kUnstuffThreads)
    reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(buf)[i];
  if (end_full < first_full) {  // the tile's bytes lie inside one chunk
    if (t >= head && t < stop) dst[t] = buf[t];
  } else {
    if (t < 16 && t >= head && first_full > 0) dst[t] = buf[t];              // chunk shared with the previous tile
    if (t < (stop & 15)) dst[end_full * 16 + t] = buf[end_full * 16 + t];  // chunk shared with the next tile
  }
  return total;
}

// The scan's bookkeeping once its length is known: split-marker overflow, restart-interval ends; the
// padding of an empty scan.
__device__ void us_finish(ImgDesc* d, const SegView& sv, int t, int64_t ulen, int nsplit, int end_code,
                          int64_t end_raw, uint8_t* out) {
  if (t == 0) {
    d->ulen = ulen;
    d->useg_found = 1 + nsplit;
    d->scan_end_code = end_code;
    d->scan_end_raw = end_raw;
    if (nsplit > sv.cap) d->status = SDSJ_CORRUPT;  // more split markers than slots
  }
  if (d->ntiles == 0)  // no entropy-coded data: an empty stream and its padding
    for (int i = t; i < (kUPad >> 4); i += kUnstuffThreads) reinterpret_cast<uint4*>(out)[i] = make_uint4(0, 0, 0, 0);
  const int nseg = d->nseg;
  const int64_t bps = d->restart_interval ? (int64_t)d->restart_interval * d->bpm : d->total_blocks;
  for (int k = t; k < nseg; k += kUnstuffThreads) {
    const int64_t ge = (int64_t)(k + 1) * bps;
    sv.vend[k] = (int32_t)(ge < d->total_blocks ? ge : d->total_blocks);
  }
}

// Images of at most kUsSerialTiles tiles (route kRtUsSmall): one workgroup per image, tile after tile.
// 6 waves per SIMD (80 VGPRs, from 84 at the default 5): -2 % per launch (8: 64 VGPRs with spills, +6 %;
// profiles/r05_ab.txt)
#ifndef SDSJ_US_WAVES
#define SDSJ_US_WAVES 6
#endif
#define SDSJ_US_OCC __attribute__((amdgpu_waves_per_eu(SDSJ_US_WAVES)))
__global__ void __launch_bounds__(kUnstuffThreads) SDSJ_US_OCC k_us_serial(const uint8_t* __restrict__ blob,
                                                               const int64_t* __restrict__ offsets,
                                                               ImgDesc* __restrict__ descs, uint8_t* __restrict__ scratch,
                                                               const int32_t* __restrict__ routes, int cap) {
  __shared__ alignas(16) uint8_t buf[16 + kUsTile + kUPad + 16];
  __shared__ int wsum[kUnstuffThreads / 64];
  __shared__ int wmin[kUnstuffThreads / 64];
  __shared__ int s_code;
  const int t = threadIdx.x;
  const int cnt = routes[kRtUsSmall];
  const int32_t* lst = route_list(routes, cap, kRtUsSmall);
  for (int q = blockIdx.x; q < cnt; q += gridDim.x) {
    const int img = lst[q];
    ImgDesc* d = &descs[img];
    const uint8_t* e = blob + offsets[img] + d->entropy_off;
    const int64_t L = d->entropy_len;
    const int ntiles = d->ntiles;
    uint8_t* out = scratch + d->off_ustream;  // 256-byte aligned
    const SegView sv = seg_view(scratch + d->off_seg, d->nseg);
    int64_t obase = 0, end_raw = -1;
    int nsplit = 0, end_code = -1;
    UsRaw raw;
    if (ntiles > 0) us_load(e, L, t * kUsBytes, raw);
    for (int j = 0; j < ntiles; j++) {
      const int64_t my0 = (int64_t)j * kUsTile + t * kUsBytes;
      UsClass c;
      us_classify(e, L, my0, raw, c);
      if (j + 1 < ntiles) us_load(e, L, my0 + kUsTile, raw);  // the next tile's loads fly meanwhile
      const int my_end = us_my_end(c, t);
      const int tile_end = us_tile_end(my_end, t, wmin);
      const bool ends = tile_end != kUsNone;
      if (ends && my_end == tile_end) s_code = us_end_code(c, t, tile_end);
      // (restart intervals: libjpeg-turbo decodes every MCU with decode_mcu_slow, no divergence)
      if ((c.fillstuff & us_below(tile_end, t)) && d->restart_interval == 0) d->status = SDSJ_CORRUPT;
      const int tot = us_place(c, my0, t, tile_end, obase, nsplit, ends || j == ntiles - 1, out, sv, buf, wsum);
      obase += tot & 0xFFFF;
      nsplit += tot >> 16;
      if (ends) {
        end_code = s_code;  // (written before us_place's barriers)
        end_raw = (int64_t)j * kUsTile + tile_end - 1;
        break;
      }
    }
    us_finish(d, sv, t, obase, nsplit, end_code, end_raw, out);
  }
}

// Larger images (route kRtUsBig): kUsGrid virtual workgroups per image stride over its tiles.
// Pass 1 -- per tile: bytes emitted and split markers before the tile's end, the end and its code.
__global__ void __launch_bounds__(kUnstuffThreads) k_us_count(const uint8_t* __restrict__ blob,
                                                              const int64_t* __restrict__ offsets,
                                                              ImgDesc* __restrict__ descs, uint8_t* __restrict__ scratch,
                                                              const int32_t* __restrict__ routes, int cap) {
  __shared__ int wsum[kUnstuffThreads / 64];
  __shared__ int wmin[kUnstuffThreads / 64];
  __shared__ int s_code;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int cnt = routes[kRtUsBig];
  const int32_t* lst = route_list(routes, cap, kRtUsBig);
  for (int v = blockIdx.x; v < cnt * kUsGrid; v += gridDim.x) {
    const int img = lst[v / kUsGrid];
    const ImgDesc* d = &descs[img];
    const int ntiles = d->ntiles;
    const uint8_t* e = blob + offsets[img] + d->entropy_off;
    const int64_t L = d->entropy_len;
    UsTile* tiles = reinterpret_cast<UsTile*>(scratch + d->off_tiles);
    for (int j = v % kUsGrid; j < ntiles; j += kUsGrid) {
      const int64_t my0 = (int64_t)j * kUsTile + t * kUsBytes;
      UsRaw raw;
      UsClass c;
      us_load(e, L, my0, raw);
      us_classify(e, L, my0, raw, c);
      const int my_end = us_my_end(c, t);
      const int tile_end = us_tile_end(my_end, t, wmin);
      if (tile_end != kUsNone && my_end == tile_end) s_code = us_end_code(c, t, tile_end);
      const uint32_t below = us_below(tile_end, t);
      int packed = __popc(c.emit & below) | (__popc(c.split & below) << 16);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) packed += __shfl_xor(packed, o, 64);
      if (lane == 0) wsum[wv] = packed;
      __syncthreads();
      if (t == 0) {
        int tot = 0;
#pragma unroll
        for (int q = 0; q < kUnstuffThreads / 64; q++) tot += wsum[q];
        UsTile r;
        r.emit = tot & 0xFFFF;
        r.split = tot >> 16;
        r.end = tile_end == kUsNone ? -1 : tile_end;
        r.code = tile_end == kUsNone ? -1 : s_code;
        tiles[j] = r;
      }
      __syncthreads();  // wsum, wmin and s_code read
    }
  }
}

// Pass 2 -- one workgroup per image: tile records -> {bytes before, split markers before, end,
// kUsFinal / kUsSkip / 0}; the scan's length, split count and end marker.
__global__ void __launch_bounds__(kUnstuffThreads) k_us_scan(ImgDesc* __restrict__ descs, uint8_t* __restrict__ scratch,
                                                             const int32_t* __restrict__ routes, int cap) {
  __shared__ int wsum[3][kUnstuffThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int cnt = routes[kRtUsBig];
  const int32_t* lst = route_list(routes, cap, kRtUsBig);
  for (int q = blockIdx.x; q < cnt; q += gridDim.x) {
    ImgDesc* d = &descs[lst[q]];
    const int ntiles = d->ntiles;
    const SegView sv = seg_view(scratch + d->off_seg, d->nseg);
    UsTile* tiles = reinterpret_cast<UsTile*>(scratch + d->off_tiles);
    int ebase = 0, sbase = 0, ended = 0;  // totals over the chunks before this one
    int64_t ulen = 0, end_raw = -1;
    int nsplit = 0, end_code = -1;
    for (int j0 = 0; j0 < ntiles; j0 += kUnstuffThreads) {
      const int j = j0 + t;
      const UsTile r = j < ntiles ? tiles[j] : UsTile{0, 0, -1, -1};
      const int hasend = r.end >= 0 ? 1 : 0;
      const int ie = wave_incl_scan(r.emit), is = wave_incl_scan(r.split), ih = wave_incl_scan(hasend);
      if (lane == 63) {
        wsum[0][wv] = ie;
        wsum[1][wv] = is;
        wsum[2][wv] = ih;
      }
      __syncthreads();
      int be = 0, bs = 0, bh = 0, te = 0, ts = 0, th = 0;
#pragma unroll
      for (int w = 0; w < kUnstuffThreads / 64; w++) {
        be += w < wv ? wsum[0][w] : 0;
        bs += w < wv ? wsum[1][w] : 0;
        bh += w < wv ? wsum[2][w] : 0;
        te += wsum[0][w];
        ts += wsum[1][w];
        th += wsum[2][w];
      }
      const int ends_before = ended + bh + ih - hasend;
      if (j < ntiles) {
        UsTile o;
        o.emit = ebase + be + ie - r.emit;
        o.split = sbase + bs + is - r.split;
        o.end = r.end >= 0 ? r.end : kUsNone;
        const bool final = ends_before == 0 && (hasend || j == ntiles - 1);
        o.code = ends_before > 0 ? kUsSkip : (final ? kUsFinal : 0);
        tiles[j] = o;
        if (final) {  // (one thread of the image)
          ulen = o.emit + r.emit;
          nsplit = o.split + r.split;
          end_code = hasend ? r.code : -1;
          end_raw = hasend ? (int64_t)j * kUsTile + r.end - 1 : -1;
          d->ulen = ulen;
          d->useg_found = 1 + nsplit;
          d->scan_end_code = end_code;
          d->scan_end_raw = end_raw;
          if (nsplit > sv.cap) d->status = SDSJ_CORRUPT;  // more split markers than slots
        }
      }
      ebase += te;
      sbase += ts;
      ended += th;
      __syncthreads();  // wsum read
    }
    const int nseg = d->nseg;
    const int64_t bps = d->restart_interval ? (int64_t)d->restart_interval * d->bpm : d->total_blocks;
    for (int k = t; k < nseg; k += kUnstuffThreads) {
      const int64_t ge = (int64_t)(k + 1) * bps;
      sv.vend[k] = (int32_t)(ge < d->total_blocks ? ge : d->total_blocks);
    }
  }
}

// Pass 3 -- per tile: places the bytes and markers at the offsets pass 2 found.
__global__ void __launch_bounds__(kUnstuffThreads) k_us_write(const uint8_t* __restrict__ blob,
                                                              const int64_t* __restrict__ offsets,
                                                              ImgDesc* __restrict__ descs, uint8_t* __restrict__ scratch,
                                                              const int32_t* __restrict__ routes, int cap) {
  __shared__ alignas(16) uint8_t buf[16 + kUsTile + kUPad + 16];
  __shared__ int wsum[kUnstuffThreads / 64];
  const int t = threadIdx.x;
  const int cnt = routes[kRtUsBig];
  const int32_t* lst = route_list(routes, cap, kRtUsBig);
  for (int v = blockIdx.x; v < cnt * kUsGrid; v += gridDim.x) {
    const int img = lst[v / kUsGrid];
    ImgDesc* d = &descs[img];
    if (d->status != SDSJ_OK) continue;  // (split-marker overflow found by pass 2)
    const int ntiles = d->ntiles;
    const uint8_t* e = blob + offsets[img] + d->entropy_off;
    const int64_t L = d->entropy_len;
    uint8_t* out = scratch + d->off_ustream;
    const SegView sv = seg_view(scratch + d->off_seg, d->nseg);
    const UsTile* tiles = reinterpret_cast<const UsTile*>(scratch + d->off_tiles);
    for (int j = v % kUsGrid; j < ntiles; j += kUsGrid) {
      const UsTile r = tiles[j];
      if (r.code == kUsSkip) break;  // the scan ended in an earlier tile (so it did for the later ones)
      const int64_t my0 = (int64_t)j * kUsTile + t * kUsBytes;
      UsRaw raw;
      UsClass c;
      us_load(e, L, my0, raw);
      us_classify(e, L, my0, raw, c);
      if ((c.fillstuff & us_below(r.end, t)) && d->restart_interval == 0)
        d->status = SDSJ_CORRUPT;  // FF FF .. 00 (us_classify)
      us_place(c, my0, t, r.end, r.emit, r.split, r.code == kUsFinal, out, sv, buf, wsum);
      if (r.code == kUsFinal) break;
      __syncthreads();  // buf and wsum reused
    }
  }
}

// k_scanmap: one thread per image -- restart intervals -> data segments and the markers after the scan
// (finish_scan), from what k_unstuff recorded.
__global__ void __launch_bounds__(64) k_scanmap(int n, const uint8_t* __restrict__ blob, const int64_t* __restrict__ offsets,
                                                ImgDesc* __restrict__ descs, uint8_t* __restrict__ scratch) {
  const int img = blockIdx.x * 64 + threadIdx.x;
  if (img >= n) return;
  ImgDesc* d = &descs[img];
  if (d->status != SDSJ_OK || d->progressive || d->png) return;  // progressive: k_prog reads the raw stream
  const SegView sv = seg_view(scratch + d->off_seg, d->nseg);
  finish_scan(d, sv, blob + offsets[img], d->entropy_len, d->useg_found - 1, d->scan_end_code, d->scan_end_raw, d->ulen, 0);
}

// ------------------------------------------------------------------------------------------
// Host-side launchers (called by the engine; all asynchronous on `stream`).
// ------------------------------------------------------------------------------------------
hipError_t launch_unstuff(int n, const uint8_t* blob, const int64_t* offsets, ImgDesc* descs, uint8_t* scratch,
                          const int32_t* routes, int cap, hipStream_t s, uint64_t rm, uint64_t hint) {
  const int g = n < kUsLaunch ? n : kUsLaunch;
#ifndef SDSJ_US_TILE_GRID
#define SDSJ_US_TILE_GRID 16384
#endif
  const int gt = n * kUsGrid < SDSJ_US_TILE_GRID ? n * kUsGrid : SDSJ_US_TILE_GRID;
#ifndef SDSJ_US_SERIAL_GRID
#define SDSJ_US_SERIAL_GRID 16384
#endif
  const int gs = n < SDSJ_US_SERIAL_GRID ? n : SDSJ_US_SERIAL_GRID;
  if (route_on(rm, kRtUsSmall))
    hipLaunchKernelGGL(k_us_serial, dim3(route_grid(hint, kRtUsSmall, gs)), dim3(kUnstuffThreads), 0, s, blob, offsets, descs,
                       scratch, routes, cap);
  if (route_on(rm, kRtUsBig)) {  // (the three kernels stride over their work)
    hipLaunchKernelGGL(k_us_count, dim3(route_grid(hint, kRtUsBig, gt)), dim3(kUnstuffThreads), 0, s, blob, offsets, descs,
                       scratch, routes, cap);
    hipLaunchKernelGGL(k_us_scan, dim3(route_grid(hint, kRtUsBig, g)), dim3(kUnstuffThreads), 0, s, descs, scratch, routes,
                       cap);
    hipLaunchKernelGGL(k_us_write, dim3(route_grid(hint, kRtUsBig, gt)), dim3(kUnstuffThreads), 0, s, blob, offsets, descs,
                       scratch, routes, cap);
  }
  return hipGetLastError();
}
hipError_t launch_scanmap(int n, const uint8_t* blob, const int64_t* offsets, ImgDesc* descs, uint8_t* scratch,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_scanmap, dim3((n + 63) / 64), dim3(64), 0, s, n, blob, offsets, descs, scratch);
  return hipGetLastError();
}

}  // namespace sdsj
