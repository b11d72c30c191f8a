// sdsj_scans.hip -- multi-scan sequential JPEG (SOF0 / SOF1 frames whose components arrive in more than one
// scan) for the MI355X path, under SDSJ_FORMAT_JPEG_SCANS, and every sequential frame of four components (CMYK /
// YCCK, in one interleaved scan or several) under SDSJ_FORMAT_JPEG_CMYK.
//
// Restates libjpeg-turbo's sequential Huffman decoder as Pillow runs it on such a file: jdhuff.c decode_mcu (the
// DC difference and the run/size AC symbols of every block of an MCU in one pass, no EOB runs, no successive
// approximation), jdinput.c per-scan MCU geometry and latch_quant_tables, jdmarker.c read_markers between scans
// (DHT / DQT / DRI may change) up to EOI, jdcoefct.c consume_data's full-image coefficient buffer (zeroed; a
// component no scan codes stays zero).  The scheme is k_prog's (sdsj_progressive.hip): one wave walks an image's
// whole file with its decoder state wave-uniform, through the bit reader, table derivation and restart rules of
// sdsj_scan_wave.h, and writes the int16 blocks k_idct reads for progressive images.  A kernel of its own, so that
// k_prog's code generation stays what it is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdsj_common.h"
#include "sdsj_kernels.h"
#include "sdsj_scan_wave.h"

namespace sdsj {

namespace {

// One block (jdhuff.c decode_mcu_slow's body): DC difference, then AC 1..63 as run/size symbols.  D / A: the
// lookahead tables of the scan's DC / AC tables, slot q each.  (A symbol starts with >= 32 bits in the buffer:
// its code and extra bits, <= 17 + 15, need no second check -- phuff.)
__device__ __forceinline__ void sblock(PBits& b, const PLds& D, const PLds& A, const ProgTables* __restrict__ T, int dslot,
                                       int aslot, int q, int16_t* blk, int* last_dc) {
  int s = phuff(b, D, T, dslot, q);
  if (s) s = pextend(pgetbits_nc(b, s), s);
  s += *last_dc;
  *last_dc = s;
  blk[0] = (int16_t)s;
  for (int k = 1; k < 64; k++) {
    const int sym = phuff(b, A, T, aslot, q);
    const int r = sym >> 4, n = sym & 15;
    if (n) {
      k += r;
      blk[zig(k)] = (int16_t)pextend(pgetbits_nc(b, n), n);
    } else if (r == 15) {
      k += 15;
    } else {
      break;
    }
  }
}

// Fill bytes before a stuffed zero (FF FF .. 00) in raw[i0, i1), looked for by all lanes: jdhuff.c
// jpeg_fill_bit_buffer (and pfill) reads it as one FF data byte, libjpeg-turbo's decode_mcu_fast takes the first
// FF FF for a marker and leaves other coefficients -- which of the two Pillow's run takes depends on its input
// buffering, so a scan without restart intervals (with them only the former runs) that holds it is refused, as
// k_unstuff refuses a baseline one.  Any such run ends in FF FF 00.
__device__ __forceinline__ bool fill_stuffed(const uint8_t* __restrict__ raw, int i0, int i1, int lane) {
  bool hit = false;
  for (int i = i0 + lane; i + 2 < i1; i += 64) hit |= raw[i] == 0xFF && raw[i + 1] == 0xFF && raw[i + 2] == 0;
  return __builtin_amdgcn_ballot_w64(hit) != 0;
}

// Every scan of image d, then the markers up to EOI.  Returns an SDSJ status.
__device__ __forceinline__ int decode_scans(ImgDesc* d, ImgTables* t, const uint8_t* raw, int n, int16_t* coef,
                                            ProgTables* P, PLds& D, PLds& A, int lane) {
  // table state as k_parse left it (the DHT / DQT segments before the first SOS)
  for (int q = 0; q < 4; q++) {
    P->qt_defined[q] = t->qt_defined[q];
    for (int i = 0; i < 64; i++) P->qt[q][i] = t->qt[q][i];
    for (int k = 0; k < 2; k++) {
      const HuffSpec& h = k ? t->ac_spec[q] : t->dc_spec[q];
      const int slot = k * 4 + q;
      P->defined[slot] = h.defined;
      for (int l = 0; l <= 16; l++) P->bits[slot][l] = h.bits[l];
      for (int i = 0; i < 256; i++) P->vals[slot][i] = h.vals[i];
    }
  }
  d->smooth = 0;  // (jdcoefct.c smooths progressive files only)
  int coded = 0;  // components some scan has coded
  int restart_interval = d->restart_interval;
  const int mcux = d->mcux, bpm = d->bpm, ncomp = d->ncomp;
  // first block of each component within an MCU
  const int boff1 = d->comp[0].h * d->comp[0].v, boff2 = boff1 + d->comp[1].h * d->comp[1].v;
  const int boff3 = boff2 + d->comp[2].h * d->comp[2].v;  // (the fourth component of a CMYK / YCCK frame)
  int pos = (int)d->sos_pos;
  for (;;) {
    if (pos + 2 > n) return SDSJ_CORRUPT;
    const int len = rd16(raw + pos), sl = len - 2;
    if (len < 2 || pos + len > n) return SDSJ_CORRUPT;
    const uint8_t* s = raw + pos + 2;
    if (sl < 1) return SDSJ_CORRUPT;
    const int ns = s[0];
    if (ns < 1 || ns > 4 || sl != 2 * ns + 4) return SDSJ_CORRUPT;  // get_sos: JERR_BAD_LENGTH
    if (ns > ncomp) return SDSJ_UNSUPPORTED;  // (a frame of three components: one of them would be coded twice)
    // (per-position arrays are indexed only from unrolled loops, so they stay in registers)
    int td[4] = {0, 0, 0, 0}, ta[4] = {0, 0, 0, 0}, sh[4] = {1, 1, 1, 1}, sv[4] = {1, 1, 1, 1}, sbo[4] = {0, 0, 0, 0},
        ldc[4] = {0, 0, 0, 0};
    int c0 = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (q >= ns) break;
      const int cid = s[1 + 2 * q];
      int c = 0;
      while (c < ncomp && comp_id_of(*d, c) != cid) c++;
      if (c == ncomp) return SDSJ_CORRUPT;
      const CompDesc cq = comp_of(*d, c);
      // a component coded a second time: libjpeg overlays the coefficients (and only warns)
      if ((coded >> c) & 1) return SDSJ_UNSUPPORTED;
      coded |= 1 << c;
      if (q == 0) c0 = c;
      td[q] = s[2 + 2 * q] >> 4;
      ta[q] = s[2 + 2 * q] & 15;
      sh[q] = cq.h;
      sv[q] = cq.v;
      sbo[q] = c == 0 ? 0 : c == 1 ? boff1 : c == 2 ? boff2 : boff3;
      // latch_quant_tables: the component's table at its (only) scan, into the slot k_idct reads (see EOI)
      const int tq = cq.tq;
      if (!P->qt_defined[tq]) return SDSJ_CORRUPT;
      for (int i = 0; i < 64; i++) t->qt[c][i] = P->qt[tq][i];
      if (td[q] > 3 || !pderive(P, D, td[q], q, lane)) return SDSJ_CORRUPT;
      if (ta[q] > 3 || !pderive(P, A, 4 + ta[q], q, lane)) return SDSJ_CORRUPT;
    }
    // a scan with other spectral or approximation parameters: libjpeg warns and decodes it as sequential
    if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return SDSJ_UNSUPPORTED;
    PBits b;
    b.d = raw;
    b.n = n;
    b.pos = pos + len;
    b.buf = 0;
    b.nbits = b.hit_marker = b.marker = b.pad_bits = b.insufficient = b.eof = 0;
    b.wbase = 1;  // (no window yet: never 16-byte aligned)
    int restarts_left = restart_interval, next_num = 0;
    // jdhuff.c decode_mcu before an MCU's blocks: the restart marker when one is due; then 0: decode the MCU,
    // 1: the data ran out, its coefficients stay zero (insufficient_data), -1: the input ended
    auto begin_mcu = [&]() -> int {
      if (restart_interval) {
        if (restarts_left == 0) {
          if (pprocess_restart(b, &next_num)) return -1;
          ldc[0] = ldc[1] = ldc[2] = ldc[3] = 0;
          restarts_left = restart_interval;
        }
        restarts_left--;
      }
      return b.insufficient;
    };
    if (ns == 1) {
      // jdinput.c per_scan_setup: a single-component scan walks that component's own block grid, an MCU a block
      const CompDesc cp = comp_of(*d, c0);
      const int cwb = (cp.dw + 7) / 8, chb = (cp.dh + 7) / 8;
      const int ch = sh[0], cv = sv[0], bo = sbo[0], dsl = td[0], asl = 4 + ta[0];
      for (int by = 0; by < chb; by++) {
        const int my = by / cv, rowbase = my * mcux * bpm + bo + (by - my * cv) * ch;
        for (int bx = 0; bx < cwb; bx++) {
          const int st = begin_mcu();
          if (st < 0) return SDSJ_CORRUPT;
          if (st) continue;
          const int mx = bx / ch;
          sblock(b, D, A, P, dsl, asl, 0, coef + (rowbase + mx * bpm + bx - mx * ch) * 64, &ldc[0]);
        }
      }
    } else {
      const int nmcu = mcux * d->mcuy;
      for (int m = 0; m < nmcu; m++) {
        const int st = begin_mcu();
        if (st < 0) return SDSJ_CORRUPT;
        if (st) continue;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          if (q >= ns) break;
          const int nb = sh[q] * sv[q];  // (the component's blocks are consecutive in the MCU, rows of h)
          for (int k = 0; k < nb; k++) sblock(b, D, A, P, td[q], 4 + ta[q], q, coef + (m * bpm + sbo[q] + k) * 64, &ldc[q]);
        }
      }
    }
    if (b.eof) return SDSJ_CORRUPT;  // the input ended inside the scan (Pillow: truncated)
    if (!b.hit_marker && pnext_marker(b) < 0) return SDSJ_CORRUPT;
    if (restart_interval == 0 && fill_stuffed(raw, pos + len, b.pos, lane)) return SDSJ_CORRUPT;
    // jdmarker.c read_markers until the next SOS or EOI
    for (;;) {
      if (b.pos + 1 >= n) return SDSJ_CORRUPT;
      const int m = pbyte(b, b.pos + 1);
      const int body = b.pos + 2;
      if (m == 0xD9) {
        // k_idct reads each component's latched table from slot c (a component never coded: zero blocks)
        for (int c = 0; c < ncomp && c < kMaxComp; c++) d->comp[c].tq = c;
        if (ncomp > kMaxComp) d->comp3.tq = kMaxComp;
        return SDSJ_OK;
      }
      if ((m >= 0xD0 && m <= 0xD7) || m == 0x01) {
        b.pos = body;
      } else {
        const bool seg = (m >= 0xE0 && m <= 0xEF) || m == 0xFE || m == 0xDC || m == 0xCC || m == 0xDD ||
                         m == 0xC4 || m == 0xDB || m == 0xDA;
        if (!seg) return SDSJ_CORRUPT;  // a second SOI / SOF, or an unknown marker
        if (m == 0xDC || m == 0xCC) return SDSJ_UNSUPPORTED;
        if (body + 2 > n) return SDSJ_CORRUPT;
        const int l2 = rd16(raw + body);
        if (l2 < 2 || body + l2 > n) return SDSJ_CORRUPT;
        if (m == 0xDA) {
          pos = body;
          break;
        }
        int st = SDSJ_OK;
        if (m == 0xC4) st = pread_dht(P, raw + body + 2, l2 - 2);
        if (m == 0xDB) st = pread_dqt(P, raw + body + 2, l2 - 2);
        if (m == 0xDD) {
          if (l2 != 4) return SDSJ_CORRUPT;
          restart_interval = rd16(raw + body + 2);
        }
        if (st != SDSJ_OK) return st;
        b.pos = body + l2;
      }
      if (pnext_marker(b) < 0) return SDSJ_CORRUPT;
    }
  }
}

}  // namespace

// One wave per image; the lookahead tables of the scan's DC and AC tables in LDS, one PLds each (k_prog's struct as it
// stands: its interleaved-DC fields are unused here; its fourth scan position serves four-component frames).  The registers allow 5 waves per SIMD,
// 20 per CU; the 8.2 KB of LDS per one-wave workgroup cap a CU's 160 KB at 19.
constexpr int kScansThreads = 64;
__global__ void __launch_bounds__(kScansThreads) __attribute__((amdgpu_waves_per_eu(5)))
k_scans(ImgDesc* __restrict__ descs, ImgTables* __restrict__ tables, const uint8_t* __restrict__ blob,
        const int64_t* __restrict__ offsets, const int32_t* __restrict__ lengths, uint8_t* __restrict__ scratch,
        const int32_t* __restrict__ routes, int cap) {
  __shared__ PLds lds_dc, lds_ac;
  const int cnt = routes[kRtScans];
  const int32_t* lst = route_list(routes, cap, kRtScans);
  for (int li = blockIdx.x; li < cnt; li += gridDim.x) {  // (one entry per workgroup at the full grid)
    const int img = lst[li];
    ImgDesc* d = &descs[img];
    if (d->status == SDSJ_OK) {
      const int st = decode_scans(d, &tables[img], blob + offsets[img], lengths[img],
                                  reinterpret_cast<int16_t*>(scratch + d->off_coef),
                                  reinterpret_cast<ProgTables*>(scratch + d->off_ptab), lds_dc, lds_ac, threadIdx.x);
      if (st != SDSJ_OK && threadIdx.x == 0) d->status = st;
    }
    __syncthreads();  // LDS reuse by the next entry
  }
}

hipError_t launch_scans(int n, ImgDesc* descs, ImgTables* tables, const uint8_t* blob, const int64_t* offsets,
                        const int32_t* lengths, uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s,
                        uint64_t rm, uint64_t hint) {
  if (!route_on(rm, kRtScans)) return hipSuccess;
  // (a scan stores only the non-zero coefficients of the blocks it codes: the MCU padding a single-component scan
  // skips, and components no scan codes, stay zero)
  launch_coef_zero(kRtScans, n, descs, scratch, routes, cap, s, hint);
  hipLaunchKernelGGL(k_scans, dim3(route_grid(hint, kRtScans, n)), dim3(kScansThreads), 0, s, descs, tables, blob,
                     offsets, lengths, scratch, routes, cap);
  return hipGetLastError();
}

}  // namespace sdsj
