// sdsj_idct.hip -- gfx950 (MI355X) kernel of the inverse DCT (its arithmetic: sdsj_idct.h).
//
// Stage map (reference behaviour each kernel reproduces, see DESIGN.md for the layout/rooflines):
//   k_idct     dequant + ISLOW IDCT                jidctint.c jpeg_idct_islow
//              (k_idct<kMaxComp>: every image but the four-component ones of SDSJ_FORMAT_JPEG_CMYK, which
//               k_idct<4> takes when the engine's mask has that bit)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdsj_common.h"
#include "sdsj_kernels.h"
#include "sdsj_idct.h"

#pragma clang fp contract(off)

namespace sdsj {

// ------------------------------------------------------------------------------------------
// k_idct: dequantisation + ISLOW IDCT with the SIMD version's 16-bit semantics (sdsj_idct.h); one block per
// thread, 256 blocks per iteration.
// ------------------------------------------------------------------------------------------
constexpr int kIdctThreads = 256;
#ifndef SDSJ_IDCT_GRID
#define SDSJ_IDCT_GRID 8
#endif
constexpr int kIdctGrid = SDSJ_IDCT_GRID;  // workgroups per image (each strides over 8-block groups)
// SDSJ_IDCT_GPW > 0 (0: kIdctGrid per image): batch launches take kIdctGridMax workgroups per image and an image uses
// ceil(total_blocks / 8 / SDSJ_IDCT_GPW) of them (1 .. kIdctGridMax; the rest exit at once), so a
// workgroup's setup is amortised over about the same number of groups whatever the image size.
#ifndef SDSJ_IDCT_GPW
#define SDSJ_IDCT_GPW 256
#endif
// (odd: workgroup k of the launch runs on XCD k mod 8, so with a grid row of 16 every image's first
// workgroups would land on the same XCDs; 17 rotates them by one XCD per image)
constexpr int kIdctGridMax = 17;

// The compact coefficient format's side of k_idct (sdsj_common.h coef_compact).  m: a block's 64-byte main slot
// as 16 dwords (bytes 0-1 flag | DC << 1 | AC 63 << 12, byte k + 1 = the low byte of AC k, k = 1..62); h: a
// flagged block's hi slot (byte k = AC k's part beyond its low byte; AC 63's beyond its 4 bits: bytes 0 and 63).
// Any AC byte outside row 0 (zigzag positions 0, 1, 5, 6, 14, 15, 27, 28) -- a coefficient is zero iff both its
// bytes are.
__device__ __forceinline__ uint32_t coef8_ac_main(const uint32_t* m) {
  uint32_t ac = (m[0] & 0xFF00F000u) | (m[1] & 0x0000FFFFu) | m[2] | (m[3] & 0x00FFFFFFu) | (m[4] & 0xFFFFFF00u) |
                m[5] | m[6] | (m[7] & 0xFFFF0000u);
#pragma unroll
  for (int i = 8; i < 16; i++) ac |= m[i];
  return ac;
}
__device__ __forceinline__ uint32_t coef8_ac_hi(const uint32_t* h) {
  uint32_t ac = (h[0] & 0xFFFF00FFu) | (h[1] & 0xFF0000FFu) | h[2] | (h[3] & 0x0000FFFFu) | h[4] | h[5] |
                (h[6] & 0x00FFFFFFu) | (h[7] & 0xFFFFFF00u);
#pragma unroll
  for (int i = 8; i < 16; i++) ac |= h[i];
  return ac;
}
// Dequantisation straight from the byte extracts: AC k = sext8(main byte k + 1), plus (sext8(hi byte k) << 8)
// wrapped to 16 bits for a flagged block (WIDE); AC 63 = its 4 bits of the first word, plus 16 x (hi bytes 0
// and 63 as an int16) when flagged.  DC = dcv.  q: the component's table in zigzag order (LDS).
template <bool WIDE>
__device__ __forceinline__ void dequant8(const uint32_t* m, const uint32_t* h, const int32_t* q, int dcv, int* x) {
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int4 qv = *reinterpret_cast<const int4*>(&q[i * 4]);
    const int qq[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int k = i * 4 + j;
      int cv;
      if (k == 0) cv = dcv;
      else if (k == 63) cv = __builtin_amdgcn_sbfe((int)m[0], 12, 4);
      else cv = __builtin_amdgcn_sbfe((int)m[(k + 1) >> 2], 8 * ((k + 1) & 3), 8);
      if (WIDE && k == 63)
        cv = (int)(int16_t)(cv + ((__builtin_amdgcn_sbfe((int)h[0], 0, 8) + (__builtin_amdgcn_sbfe((int)h[15], 24, 8) << 8)) << 4));
      else if (WIDE && k > 0) cv = (int)(int16_t)(cv + (__builtin_amdgcn_sbfe((int)h[i], 8 * j, 8) << 8));
      x[natural_order(k)] = wrap16(cv * qq[j]);
    }
  }
}

// Work unit = a group: 8 horizontally adjacent blocks of one component, one per thread, so each of
// a block's 8 row stores joins the group's other 7 in 64 contiguous bytes of a plane row.  The
// block stays in registers through both passes (64 values), so there is no LDS transpose.
#ifndef SDSJ_IDCT_WAVES
#define SDSJ_IDCT_WAVES 4  // waves per SIMD the register budget targets (124 VGPRs at 4)
#endif
// NC: the components the instantiation holds.  k_idct<kMaxComp> is the kernel every mask launches and leaves
// four-component images alone; k_idct<4> takes only those -- k_scans' and k_prog4's images (int16 blocks, no cut restart
// intervals), whose fourth component comes from comp_of -- and is launched only under SDSJ_FORMAT_JPEG_CMYK.
template <int NC>
__global__ void __launch_bounds__(kIdctThreads) __attribute__((amdgpu_waves_per_eu(SDSJ_IDCT_WAVES)))
k_idct(int n, const ImgDesc* __restrict__ descs,
                                                       const ImgTables* __restrict__ tables,
                                                       uint8_t* __restrict__ scratch) {
  const int img = blockIdx.y;
  if (img >= n) return;
  const ImgDesc* d = &descs[img];
  if (d->status != SDSJ_OK || d->geo == kGeoZeros || d->png) return;
  if (NC > kMaxComp ? d->ncomp != NC : d->ncomp > NC) return;
  int nwg = gridDim.x;  // this image's workgroups
  if (SDSJ_IDCT_GPW > 0 && gridDim.x == kIdctGridMax) {
    const int64_t want = ((int64_t)d->total_blocks / 8 + SDSJ_IDCT_GPW - 1) / SDSJ_IDCT_GPW;
    nwg = want < 1 ? 1 : (want > kIdctGridMax ? kIdctGridMax : (int)want);
    if ((int)blockIdx.x >= nwg) return;
  }
  __shared__ alignas(16) int32_t qt[NC][64];
  __shared__ int32_t binv[NC][16];  // (dy * 4 + dx) -> MCU block index b (jdcoefct order)
  __shared__ int32_t gstart[NC + 1], ngx[NC], cbw[NC], ch_[NC], cv_[NC], cpitch[NC];
  __shared__ int32_t cgx0[NC], cby0[NC];  // first 8-block group column / block row needed
  __shared__ float rngx[NC], rch[NC], rcv[NC];  // reciprocals for the exact quotients below
  __shared__ int64_t cplane[NC];
  const int t = threadIdx.x;
  const int ncomp = d->ncomp, bpm = d->bpm, mcux = d->mcux;
  // quantisation tables in zigzag order (the coefficient blocks' order)
  if constexpr (NC > kMaxComp) {
    for (int i = t; i < ncomp * 64; i += kIdctThreads) qt[i / 64][i % 64] = tables[img].qt[comp_of(*d, i / 64).tq][natural_order(i % 64)];
  } else {
    for (int i = t; i < ncomp * 64; i += kIdctThreads) qt[i / 64][i % 64] = tables[img].qt[d->comp[i / 64].tq][natural_order(i % 64)];
  }
  if (t < bpm) binv[d->blk_comp[t]][d->blk_dy[t] * 4 + d->blk_dx[t]] = t;
  if (t == 0) {
    // only the blocks whose pixels the colour/resample passes read (comp_block_rect: the crop's source
    // rectangle widened by one sample), in groups of 8 horizontally adjacent blocks aligned to 8 block
    // columns, so each group's row stores fill whole 64-byte plane segments (groups starting at the
    // first needed block column instead: k_idct 4.70 -> 5.18 ms per 16,384, profiles/r05_ab.txt)
    int acc = 0;
    for (int c = 0; c < ncomp; c++) {
      const CompDesc cd4 = NC > kMaxComp ? comp_of(*d, c) : CompDesc();
      const CompDesc& cd = NC > kMaxComp ? cd4 : d->comp[c];
      int bx0, bx1, by0, by1;
      const bool any = comp_block_rect(*d, cd, bx0, bx1, by0, by1);
      gstart[c] = acc;
      cgx0[c] = bx0 >> 3;
      ngx[c] = (bx1 >> 3) - cgx0[c] + 1;
      cby0[c] = by0;
      cbw[c] = cd.bw;
      ch_[c] = ncomp == 1 ? 1 : cd.h;
      cv_[c] = ncomp == 1 ? 1 : cd.v;
      cpitch[c] = cd.pitch;
      cplane[c] = cd.plane_off;
      rngx[c] = 1.0f / (float)ngx[c];
      rch[c] = 1.0f / (float)ch_[c];
      rcv[c] = 1.0f / (float)cv_[c];
      acc += any ? ngx[c] * (by1 - by0 + 1) : 0;
    }
    gstart[ncomp] = acc;
  }
  __syncthreads();
  const int lb = t & 7;  // this lane's block within its group
  // coefficient blocks (sdsj_common.h coef_compact): 64-byte main slots with the dc and hi sub-regions, or
  // 128-byte int16 blocks
  // (evaluated by every wave, on its scalar unit from the descriptor: the value stays in an SGPR and the format
  // branch below stays uniform.  Held in LDS instead, once per workgroup, the branch became a vector one and
  // k_idct went 15.6 -> 24.4 ms per 65,536)
  const bool compact = NC > kMaxComp ? false : coef_compact(*d);
  const uint8_t* coef = scratch + d->off_coef;
  const int16_t* cdc = reinterpret_cast<const int16_t*>(coef + coef_dc_off(d->total_blocks));
  const uint8_t* chi = coef + coef_hi_off(d->total_blocks);
  uint8_t* planes = scratch + d->off_planes;
  const int ngroups = gstart[ncomp];
  // blocks the entropy decoder left zero (jdhuff.c insufficient_data): from vend[k] to the end of
  // restart interval k, and all of an empty interval entered out of data
  const SegView sv = seg_view(scratch + d->off_seg, d->nseg);
  const int nseg = d->nseg;
  const int bps = d->restart_interval ? d->restart_interval * bpm : (int)d->total_blocks;
  const int vend0 = d->progressive ? 0 : sv.vend[0];
  const bool prog = d->progressive != 0;  // (k_prog decodes every block; no cut intervals)
  auto zero_block = [&](int g) {
    if (prog) return false;
    if (nseg == 1) return g >= vend0;
    const int k = g / bps;
    return g >= sv.vend[k] || (k > 0 && (sv.flag[k] & kSegEmpty) && (sv.flag[k - 1] & kSegIns));
  };
  // a / b for 0 <= a < 2^22, 1 <= b: float estimate, then one correction each way (exact)
  auto qdiv = [](int a, int b, float rb) {
    int q = (int)((float)a * rb);
    q -= q * b > a ? 1 : 0;
    q += (q + 1) * b <= a ? 1 : 0;
    return q;
  };
  // block lb of group grp: component, block coordinates, decode-order index (g < 0: none)
  auto locate = [&](int grp, int& c, int& by, int& bx, int& g) {
    c = ncomp > 1 && grp >= gstart[1] ? (ncomp > 2 && grp >= gstart[2] ? 2 : 1) : 0;
    if constexpr (NC > kMaxComp) c = grp >= gstart[kMaxComp] ? kMaxComp : c;
    const int local = grp - gstart[c];
    const int byl = qdiv(local, ngx[c], rngx[c]);
    by = cby0[c] + byl;
    bx = (cgx0[c] + local - byl * ngx[c]) * 8 + lb;
    g = -1;
    if (grp < ngroups && bx < cbw[c]) {
      const int h = ch_[c], v = cv_[c];
      const int mx = qdiv(bx, h, rch[c]), my = qdiv(by, v, rcv[c]);
      g = (my * mcux + mx) * bpm + binv[c][(by - my * v) * 4 + (bx - mx * h)];
    }
  };
  // One block per lane, held in registers: dequantise, columns (pass 1), rows (pass 2), each row's 8
  // bytes stored straight to the plane -- no LDS transposes.  The 8 lanes of a group write 64
  // contiguous bytes of a plane row per store.
  for (int grp = blockIdx.x * (kIdctThreads / 8) + (t >> 3); grp < ngroups; grp += nwg * (kIdctThreads / 8)) {
    int c, by, bx, g;
    locate(grp, c, by, bx, g);
    if (g < 0) continue;
    // the block (zigzag order), or zeros where the entropy decoder left it zero, dequantised as vpmullw does:
    // the low 16 bits of coef * quantval, zigzag position k into row-major natural_order(k).  `ac`: any raw
    // coefficient outside row 0 (the SIMD pass 1's zero test)
    const bool zb = zero_block(g);
    int x[64];
    uint32_t ac;
    if (compact) {
      // k_entwrite<11>'s 64-byte main slot; a flagged block's DC and hi slot too (rare, divergent)
      const uint4* src = reinterpret_cast<const uint4*>(coef + (int64_t)g * kCoefMain);
      uint32_t m[16];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint4 v = zb ? make_uint4(0, 0, 0, 0) : src[i];
        m[4 * i] = v.x, m[4 * i + 1] = v.y, m[4 * i + 2] = v.z, m[4 * i + 3] = v.w;
      }
      ac = coef8_ac_main(m);
      if (m[0] & 1u) {
        const int dcv = cdc[g];
        const uint4* hs = reinterpret_cast<const uint4*>(chi + (int64_t)g * kCoefMain);
        uint32_t h[16];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const uint4 v = hs[i];
          h[4 * i] = v.x, h[4 * i + 1] = v.y, h[4 * i + 2] = v.z, h[4 * i + 3] = v.w;
        }
        ac |= coef8_ac_hi(h);
        dequant8<true>(m, h, qt[c], dcv, x);
      } else {
        dequant8<false>(m, m, qt[c], __builtin_amdgcn_sbfe((int)m[0], 1, 11), x);
      }
    } else {
      // 128-byte int16 blocks (k_entwrite<10> / k_prog)
      const uint4* src = reinterpret_cast<const uint4*>(coef + (int64_t)g * kCoefFull);
      uint4 raw[8];
#pragma unroll
      for (int i = 0; i < 8; i++) raw[i] = zb ? make_uint4(0, 0, 0, 0) : src[i];
      // row 0 is zigzag positions 0, 1, 5, 6, 14, 15, 27 and 28
      ac = raw[0].y | (raw[0].z & 0xFFFFu) | (raw[0].w & 0xFFFF0000u) | raw[1].x | raw[1].y | raw[1].z |
           raw[3].x | (raw[3].y & 0xFFFFu) | (raw[3].z & 0xFFFF0000u) | raw[3].w;
#pragma unroll
      for (int i = 2; i < 8; i++) ac |= i == 3 ? 0u : (raw[i].x | raw[i].y | raw[i].z | raw[i].w);
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int4 q0 = *reinterpret_cast<const int4*>(&qt[c][i * 8]), q1 = *reinterpret_cast<const int4*>(&qt[c][i * 8 + 4]);
        const uint32_t w[4] = {raw[i].x, raw[i].y, raw[i].z, raw[i].w};
        const int q[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const int cv = (int)(int16_t)((w[k >> 1] >> ((k & 1) * 16)) & 0xFFFF);
          x[natural_order(i * 8 + k)] = wrap16(cv * q[k]);
        }
      }
    }
    // pass 1: columns.  A block whose rows 1..7 are all zero takes the SIMD shortcut (vpsllw: every
    // column is the dequantised DC << PASS1_BITS, wrapped to 16 bits); otherwise every column runs the
    // butterfly, saturated to 16 bits.  On such a block the butterfly of column k gives sat16(4 x[k]) in
    // every row, so the shortcut is the butterfly on x[k] = wrap16(4 x[k]) / 4 (exact: a multiple of 4).
    if (!ac) {
#pragma unroll
      for (int k = 0; k < 8; k++) x[k] = wrap16(x[k] * 4) >> 2;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
      uint32_t o[8];
      islow_1d(x[k], x[8 + k], x[16 + k], x[24 + k], x[32 + k], x[40 + k], x[48 + k], x[56 + k], o);
#pragma unroll
      for (int j = 0; j < 8; j++) x[j * 8 + k] = descale_p1(o[j]);
    }
    // pass 2: rows -> 8 bytes of plane row by * 8 + r
    uint8_t* dst = planes + cplane[c] + (int64_t)(by * 8) * cpitch[c] + bx * 8;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      uint32_t o[8];
      islow_1d(x[r * 8], x[r * 8 + 1], x[r * 8 + 2], x[r * 8 + 3], x[r * 8 + 4], x[r * 8 + 5], x[r * 8 + 6], x[r * 8 + 7], o);
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) lo |= descale_p2(o[k]) << (8 * k);
#pragma unroll
      for (int k = 0; k < 4; k++) hi |= descale_p2(o[k + 4]) << (8 * k);
      *reinterpret_cast<uint2*>(dst + (int64_t)r * cpitch[c]) = make_uint2(lo, hi);
    }
  }
}

// ------------------------------------------------------------------------------------------
// Host-side launchers (called by the engine; all asynchronous on `stream`).
// ------------------------------------------------------------------------------------------
hipError_t launch_idct(int n, const ImgDesc* descs, const ImgTables* tables, uint8_t* scratch, hipStream_t s) {
  // (a few images: more workgroups per image, for latency)
  hipLaunchKernelGGL(k_idct<kMaxComp>, dim3(n <= kSmallBatch ? 8 * kIdctGrid : (SDSJ_IDCT_GPW > 0 ? kIdctGridMax : kIdctGrid), n), dim3(kIdctThreads), 0, s, n, descs,
                     tables, scratch);
  return hipGetLastError();
}
// (grid rows = the lane's images, as for k_idct: a row whose image has not four components exits at once)
hipError_t launch_idct4(int n, const ImgDesc* descs, const ImgTables* tables, uint8_t* scratch, hipStream_t s, uint64_t rm) {
  if (!route_on(rm, kRtScans) && !route_on(rm, kRtProg4)) return hipSuccess;  // (sequential and progressive ones)
  hipLaunchKernelGGL(k_idct<4>, dim3(kIdctGrid, n), dim3(kIdctThreads), 0, s, n, descs, tables, scratch);
  return hipGetLastError();
}

}  // namespace sdsj
