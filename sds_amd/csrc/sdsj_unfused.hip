// sdsj_unfused.hip -- gfx950 (MI355X) kernels of the unfused colour and resample passes.
//
// Stage map (reference behaviour each kernel reproduces, see DESIGN.md for the layout/rooflines):
//   k_color    upsampling + YCbCr->RGB (or RGB kept) jdsample.c / jdmainct.c / jdcolor.c
//   k_cmyk     upsampling + YCCK->CMYK + CMYK->RGB  jdsample.c / jdcolor.c ycck_cmyk_convert / Pillow Unpack.c
//              (four-component images)             "CMYK;I", Convert.c cmyk2rgb
//   k_coeffs   resampling tables (doubles)        Pillow Resample.c precompute_coeffs
//   k_hpass    horizontal pass, uint8 out         Pillow ImagingResampleHorizontal_8bpc
//   k_vpass    vertical pass + hflip + layout/LUT Pillow ImagingResampleVertical_8bpc,
//                                                 functional.py:102-110, presets.py:154-162
//   (k_color / k_hpass / k_vpass only run for images with fused = 0; the others, and every
//    failed sample, go through k_resample in sdsj_resample.hip)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdsj_common.h"
#include "sdsj_kernels.h"

#pragma clang fp contract(off)

namespace sdsj {

// ------------------------------------------------------------------------------------------
// k_color: upsampling (jdsample.c, context rows per jdmainct.c) + ycc_rgb_convert, or no conversion
// for an RGB-coded image.
// One thread per RGB pixel of rows [src_y0, src_y1) x cols [src_x0, src_x0 + src_w).
// ------------------------------------------------------------------------------------------
// v / r for an upsampling ratio r = 1..4 (jdsample.c int_upsample's replication): shifts, or a
// multiplication by the constant reciprocal for 3 -- no division by a variable.
__device__ __forceinline__ int ratio_div(int v, int r) { return r == 1 ? v : r == 2 ? v >> 1 : r == 4 ? v >> 2 : v / 3; }

// jdsample.c jinit_upsampler, per component: copy (1, 1), the fancy methods for (2, 1), (2, 2) and (1, 2),
// int_upsample for every other ratio (a 3 or 4 on either axis; SDSJ_FORMAT_JPEG_EXT images only).
__device__ __forceinline__ int up_sample(const uint8_t* P, const CompDesc& c, int x, int y) {
  if (c.rh == 1 && c.rv == 1) return P[(int64_t)y * c.pitch + x];
  if (c.rh > 2 || c.rv > 2) return P[(int64_t)ratio_div(y, c.rv) * c.pitch + ratio_div(x, c.rh)];  // int_upsample
  const int dw = c.dw, dh = c.dh;
  if (c.rv == 2) {
    const int i = y >> 1;
    int f = (y & 1) ? i + 1 : i - 1;
    f = f < 0 ? 0 : (f > dh - 1 ? dh - 1 : f);
    const uint8_t* r0 = P + (int64_t)i * c.pitch;
    const uint8_t* r1 = P + (int64_t)f * c.pitch;
    if (c.rh == 2) {
      const int jx = x >> 1;
      if (dw <= 2) return P[(int64_t)i * c.pitch + jx];  // h2v2_upsample (box)
      const int cs = r0[jx] * 3 + r1[jx];
      if ((x & 1) == 0) {
        const int k = jx > 0 ? jx - 1 : 0;
        const int cn = jx > 0 ? r0[k] * 3 + r1[k] : cs;
        return (cs * 3 + cn + 8) >> 4;
      } else {
        const int k = jx < dw - 1 ? jx + 1 : dw - 1;
        const int cn = jx < dw - 1 ? r0[k] * 3 + r1[k] : cs;
        return (cs * 3 + cn + 7) >> 4;
      }
    }
    // h1v2_fancy_upsample
    return (r0[x] * 3 + r1[x] + ((y & 1) ? 2 : 1)) >> 2;
  }
  // rh == 2, rv == 1: h2v1
  const uint8_t* row = P + (int64_t)y * c.pitch;
  const int jx = x >> 1;
  const int a = row[jx];
  if (dw <= 2) return a;
  if ((x & 1) == 0) return jx == 0 ? a : (a * 3 + row[jx - 1] + 1) >> 2;
  return jx == dw - 1 ? a : (a * 3 + row[jx + 1] + 2) >> 2;
}

__device__ __forceinline__ uint32_t clamp255(int v) { return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

__device__ __forceinline__ void ycc_to_rgb(int y, int cb, int cr, uint32_t* r, uint32_t* g, uint32_t* b) {
  // jdcolor.c tables evaluated arithmetically (identical integer results)
  const int x_cb = cb - 128, x_cr = cr - 128;
  const int cr_r = (91881 * x_cr + 32768) >> 16;
  const int cb_b = (116130 * x_cb + 32768) >> 16;
  const int g_add = (-46802 * x_cr + (-22554 * x_cb + 32768)) >> 16;
  *r = clamp255(y + cr_r);
  *g = clamp255(y + g_add);
  *b = clamp255(y + cb_b);
}

__global__ void __launch_bounds__(256) k_color(int n, const ImgDesc* __restrict__ descs, uint8_t* __restrict__ scratch,
                                               const int32_t* __restrict__ routes, int cap) {
 const int32_t* rl = route_list(routes, cap, kRtUnfused);
 for (int li = blockIdx.y; li < routes[kRtUnfused]; li += gridDim.y) {
  const int img = rl[li];
  const ImgDesc* d = &descs[img];
  // (PNG rows: k_png_unfilter; four components: k_cmyk)
  if (d->status != SDSJ_OK || d->geo == kGeoZeros || d->fused || d->png || d->ncomp > kMaxComp) continue;
  const int w = d->src_w, h = d->src_y1 - d->src_y0;
  const int64_t total = (int64_t)w * h;
  const uint8_t* planes = scratch + d->off_planes;
  uint8_t* rgb = scratch + d->off_rgb;
  const bool rgbc = rgb_coded(*d);  // the planes are R, G, B (jdcolor.c rgb_rgb_convert)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int yy = (int)(i / w), xx = (int)(i - (int64_t)yy * w);
    const int x = d->src_x0 + xx, y = d->src_y0 + yy;
    uint32_t R, G, B;
    const int Y = up_sample(planes + d->comp[0].plane_off, d->comp[0], x, y);
    if (d->ncomp == 1) {
      R = G = B = (uint32_t)Y;
    } else {
      const int cb = up_sample(planes + d->comp[1].plane_off, d->comp[1], x, y);
      const int cr = up_sample(planes + d->comp[2].plane_off, d->comp[2], x, y);
      if (rgbc) {
        R = (uint32_t)Y;
        G = (uint32_t)cb;
        B = (uint32_t)cr;
      } else {
        ycc_to_rgb(Y, cb, cr, &R, &G, &B);
      }
    }
    uint8_t* o = rgb + i * 3;
    o[0] = (uint8_t)R;
    o[1] = (uint8_t)G;
    o[2] = (uint8_t)B;
  }
 }
}

// ------------------------------------------------------------------------------------------
// k_cmyk<RT>: k_color's counterpart for the four-component images of SDSJ_FORMAT_JPEG_CMYK (ncomp == 4) on route RT's
// list -- kRtScans: sequential files, kRtProg4: progressive ones (SDSJ_FORMAT_JPEG_CMYK_PROG), the same code over another list:
// the RGB rows [src_y0, src_y1) x [src_x0, src_x0 + src_w) at off_rgb, as PIL.Image.open(...).convert("RGB") has
// them.  Per pixel: the four planes upsampled as jinit_upsampler chooses per component (up_sample; K too); for YCCK
// (an Adobe marker whose transform is not 0: default_decompress_parms) the first three through jdcolor.c
// ycck_cmyk_convert -- C, M, Y = 255 - R, G, B of ycc_rgb_convert, K kept --; all four inverted, as Pillow unpacks
// every four-layer JPEG ("CMYK;I"); then Convert.c cmyk2rgb: nk = 255 - K, out = clip8(nk - MULDIV255(C, nk)).
// One thread per group of four consecutive pixels of the packed rows: 12 bytes, three aligned 32-bit stores (the
// rows start 256-aligned); a component stored at full resolution is read 32 bits at a time where the group lies
// in one row at an aligned column.  The last, partial group stores bytes.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int muldiv255(int a, int b) {
  const int t = a * b + 128;
  return ((t >> 8) + t) >> 8;
}

__device__ __forceinline__ void up_sample4(const uint8_t* P, const CompDesc& c, int x, int y, bool row4, int* o) {
  if (row4 && c.rh == 1 && c.rv == 1) {  // (x % 4 == 0, pitch % 8 == 0, the plane 256-aligned)
    const uint32_t v = *reinterpret_cast<const uint32_t*>(P + (int64_t)y * c.pitch + x);
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = (int)((v >> (8 * k)) & 255u);
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) o[k] = up_sample(P, c, x + k, y);
}

template <int RT>
__global__ void __launch_bounds__(256) k_cmyk(const ImgDesc* __restrict__ descs, uint8_t* __restrict__ scratch,
                                              const int32_t* __restrict__ routes, int cap) {
 const int32_t* rl = route_list(routes, cap, RT);
 for (int li = blockIdx.y; li < routes[RT]; li += gridDim.y) {
  const ImgDesc* d = &descs[rl[li]];
  if (d->status != SDSJ_OK || d->geo == kGeoZeros || d->ncomp != 4) continue;  // (k_scans may have refused it)
  const int w = d->src_w, h = d->src_y1 - d->src_y0;
  const int64_t total = (int64_t)w * h, groups = (total + 3) >> 2;
  const uint8_t* planes = scratch + d->off_planes;
  uint8_t* rgb = scratch + d->off_rgb;
  const bool ycck = d->saw_adobe && d->adobe_transform != 0;
  const CompDesc c0 = d->comp[0], c1 = d->comp[1], c2 = d->comp[2], c3 = comp_of(*d, 3);
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = g * 4;
    const int yy = (int)(i / w), xx = (int)(i - (int64_t)yy * w);
    const int x = d->src_x0 + xx, y = d->src_y0 + yy;
    const bool full = i + 4 <= total, row = xx + 4 <= w;
    int s[4][4];  // [component][pixel of the group]
    if (full && row) {
      const bool row4 = (x & 3) == 0;
      up_sample4(planes + c0.plane_off, c0, x, y, row4, s[0]);
      up_sample4(planes + c1.plane_off, c1, x, y, row4, s[1]);
      up_sample4(planes + c2.plane_off, c2, x, y, row4, s[2]);
      up_sample4(planes + c3.plane_off, c3, x, y, row4, s[3]);
    } else {
      for (int k = 0; k < 4; k++) {
        const int64_t ik = i + k < total ? i + k : total - 1;  // (a pixel past the end repeats the last; never stored)
        const int yk = (int)(ik / w), xk = d->src_x0 + (int)(ik - (int64_t)yk * w);
        s[0][k] = up_sample(planes + c0.plane_off, c0, xk, d->src_y0 + yk);
        s[1][k] = up_sample(planes + c1.plane_off, c1, xk, d->src_y0 + yk);
        s[2][k] = up_sample(planes + c2.plane_off, c2, xk, d->src_y0 + yk);
        s[3][k] = up_sample(planes + c3.plane_off, c3, xk, d->src_y0 + yk);
      }
    }
    uint32_t px[12];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      int C = s[0][k], M = s[1][k], Y = s[2][k];
      if (ycck) {
        uint32_t R, G, B;
        ycc_to_rgb(C, M, Y, &R, &G, &B);
        C = 255 - (int)R;
        M = 255 - (int)G;
        Y = 255 - (int)B;
      }
      const int nk = s[3][k];  // 255 - (255 - K): the inverted K, complemented
      px[3 * k] = clamp255(nk - muldiv255(255 - C, nk));
      px[3 * k + 1] = clamp255(nk - muldiv255(255 - M, nk));
      px[3 * k + 2] = clamp255(nk - muldiv255(255 - Y, nk));
    }
    uint8_t* o = rgb + i * 3;
    if (full) {
      uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
      for (int q = 0; q < 3; q++)
        o32[q] = px[4 * q] | (px[4 * q + 1] << 8) | (px[4 * q + 2] << 16) | (px[4 * q + 3] << 24);
    } else {
      for (int k = 0; k < 12 && i * 3 + k < total * 3; k++) o[k] = (uint8_t)px[k];
    }
  }
 }
}

// ------------------------------------------------------------------------------------------
// k_coeffs: Pillow precompute_coeffs + normalize_coeffs_8bpc for both passes (doubles).
// ------------------------------------------------------------------------------------------
__device__ double filt_eval(int filter, double x) {
  switch (filter) {
    case SDSJ_FILTER_BOX:
      return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    case SDSJ_FILTER_BILINEAR:
      if (x < 0.0) x = -x;
      return x < 1.0 ? 1.0 - x : 0.0;
    case SDSJ_FILTER_HAMMING:
      if (x < 0.0) x = -x;
      if (x == 0.0) return 1.0;
      if (x >= 1.0) return 0.0;
      x = x * M_PI;
      return sin(x) / x * (0.54 + 0.46 * cos(x));
    case SDSJ_FILTER_BICUBIC: {
      const double a = -0.5;
      if (x < 0.0) x = -x;
      if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
      if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
      return 0.0;
    }
    default: {
      if (!(-3.0 <= x && x < 3.0)) return 0.0;
      double s1 = x == 0.0 ? 1.0 : sin(x * M_PI) / (x * M_PI);
      double x3 = x / 3;
      double s2 = x3 == 0.0 ? 1.0 : sin(x3 * M_PI) / (x3 * M_PI);
      return s1 * s2;
    }
  }
}

// NEAREST: one tap of weight 1.0 (ksize 1) at the source index of Pillow's running sum, or none (fill
// value 0).  One thread walks the whole axis (the running sum is sequential; a per-index restart
// would cost O(out^2)).
__device__ void nearest_axis(int in_size, int out_size, int32_t* bounds, int32_t* kk) {
  const double a = (double)in_size / out_size;
  double xo = 0.0 + a * 0.5;
  for (int xx = 0; xx < out_size; xx++, xo += a) {
    const int xin = xo < 0.0 ? -1 : (int)xo;
    const int s = (xin >= 0 && xin < in_size) ? xin : -1;
    kk[xx] = 1 << 22;
    bounds[2 * xx] = s < 0 ? 0 : s;
    bounds[2 * xx + 1] = s < 0 ? 0 : 1;
  }
}

__device__ void coeffs_one(int in_size, int out_size, int filter, int ksize, int xx, int32_t* bounds, int32_t* kk) {
  if (filter == SDSJ_FILTER_NEAREST) {
    if (xx == 0) nearest_axis(in_size, out_size, bounds, kk);
    return;
  }
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = filter_support(filter) * filterscale;
  const double center = 0.0 + (xx + 0.5) * scale;
  double ww = 0.0;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  double w[64];
  int32_t* k = kk + (int64_t)xx * ksize;
  // two passes: the weights are recomputed rather than stored when ksize > 64
  for (int x = 0; x < xmax; x++) {
    double v = filt_eval(filter, (x + xmin - center + 0.5) * ss);
    if (x < 64) w[x] = v;
    ww += v;
  }
  for (int x = 0; x < xmax; x++) {
    double v = x < 64 ? w[x] : filt_eval(filter, (x + xmin - center + 0.5) * ss);
    if (ww != 0.0) v /= ww;
    double s = v * (double)(1 << 22);
    k[x] = v < 0 ? (int32_t)(-0.5 + s) : (int32_t)(0.5 + s);
  }
  for (int x = xmax; x < ksize; x++) k[x] = 0;
  bounds[2 * xx] = xmin;
  bounds[2 * xx + 1] = xmax;
}

__global__ void __launch_bounds__(256) k_coeffs(int n, ImgDesc* __restrict__ descs, sdsj_op op,
                                                uint8_t* __restrict__ scratch) {
  const int img = blockIdx.y;
  if (img >= n) return;
  ImgDesc* d = &descs[img];
  if (d->status != SDSJ_OK || d->geo != kGeoResize) return;
  // an image whose crop and passes equal the lane's first image's uses that image's tables (same
  // inputs, same Pillow coefficients): most batches hold one source size
  if (img > 0) {
    const ImgDesc* a = &descs[0];
    if (a->status == SDSJ_OK && a->geo == kGeoResize && a->cw == d->cw && a->ch == d->ch && a->need_h == d->need_h &&
        a->need_v == d->need_v && a->ksh == d->ksh && a->ksv == d->ksv) {
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        d->off_kh = a->off_kh;  // (absolute scratch offsets after k_plan_apply)
        d->off_kv = a->off_kv;
      }
      return;
    }
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (d->need_h && i < op.out_w) {
    int32_t* b = reinterpret_cast<int32_t*>(scratch + d->off_kh);
    coeffs_one(d->cw, op.out_w, op.filter, d->ksh, i, b, b + 2 * op.out_w);
  }
  if (d->need_v && i < op.out_h) {
    int32_t* b = reinterpret_cast<int32_t*>(scratch + d->off_kv);
    coeffs_one(d->ch, op.out_h, op.filter, d->ksv, i, b, b + 2 * op.out_h);
  }
}

__device__ __forceinline__ uint32_t clip8(int32_t v) {
  v >>= 22;
  return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// ------------------------------------------------------------------------------------------
// k_hpass: rows [yf, yl) of the crop, out_w columns; taps clamp to the crop window.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_hpass(int n, const ImgDesc* __restrict__ descs, sdsj_op op,
                                               uint8_t* __restrict__ scratch, const int32_t* __restrict__ routes, int cap) {
 const int32_t* rl = route_list(routes, cap, kRtUnfused);
 for (int li = blockIdx.y; li < routes[kRtUnfused]; li += gridDim.y) {
  const int img = rl[li];
  const ImgDesc* d = &descs[img];
  if (d->status != SDSJ_OK || !d->need_h || d->fused) continue;
  const int rows = d->yl - d->yf, ow = op.out_w;
  const int64_t total = (int64_t)rows * ow;
  const int32_t* bounds = reinterpret_cast<const int32_t*>(scratch + d->off_kh);
  const int32_t* kk = bounds + 2 * ow;
  const uint8_t* rgb = scratch + d->off_rgb;
  uint8_t* tmp = scratch + d->off_tmp;
  const int sw = d->rgb_pitch, ks = d->ksh;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int yy = (int)(i / ow), xx = (int)(i - (int64_t)yy * ow);
    const int xmin = bounds[2 * xx], xmax = bounds[2 * xx + 1];
    const int32_t* k = kk + (int64_t)xx * ks;
    const uint8_t* row = rgb + ((int64_t)yy * sw + xmin) * 3;
    int32_t s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    for (int x = 0; x < xmax; x++) {
      const int32_t c = k[x];
      s0 += row[3 * x] * c;
      s1 += row[3 * x + 1] * c;
      s2 += row[3 * x + 2] * c;
    }
    uint8_t* o = tmp + i * 3;
    o[0] = (uint8_t)clip8(s0);
    o[1] = (uint8_t)clip8(s1);
    o[2] = (uint8_t)clip8(s2);
  }
 }
}

// ------------------------------------------------------------------------------------------
// k_vpass: vertical pass (or copy) + hflip + CHW/HWC layout + uint8 / float32 LUT output.
// Failed samples get zeros.  Also publishes the per-sample status.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_vpass(int n, const ImgDesc* __restrict__ descs, sdsj_op op,
                                               const uint8_t* __restrict__ scratch, const uint8_t* __restrict__ flip,
                                               void* __restrict__ out, const int32_t* __restrict__ routes, int cap,
                                               const float* __restrict__ lut) {
 const int32_t* rl = route_list(routes, cap, kRtUnfused);
 for (int li = blockIdx.y; li < routes[kRtUnfused]; li += gridDim.y) {
  const int img = rl[li];
  const ImgDesc* d = &descs[img];
  const int oh = op.out_h, ow = op.out_w;
  const int64_t plane = (int64_t)oh * ow;
  const int64_t total = plane;
  // failed / empty-crop images are written (and every status published) by k_finish
  if (d->status != SDSJ_OK || d->geo == kGeoZeros || d->fused) continue;
  const bool zeros = false;
  const bool fl = flip ? flip[img] != 0 : false;
  const bool f32 = op.out_dtype == SDSJ_DTYPE_F32;
  const bool hwc = op.layout == SDSJ_LAYOUT_HWC;
  uint8_t* o8 = reinterpret_cast<uint8_t*>(out) + (f32 ? 0 : img * plane * 3);
  float* of = reinterpret_cast<float*>(out) + (f32 ? img * plane * 3 : 0);
  // source: H-pass output (need_h) or the materialised RGB rows (crop columns)
  const uint8_t* src = zeros ? nullptr : (d->need_h ? scratch + d->off_tmp : scratch + d->off_rgb);
  const int sw = d->need_h ? ow : d->rgb_pitch;
  const int32_t* bounds = d->need_v ? reinterpret_cast<const int32_t*>(scratch + d->off_kv) : nullptr;
  const int32_t* kk = bounds ? bounds + 2 * oh : nullptr;
  const int ks = d->ksv, yf = d->yf;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int yy = (int)(i / ow), xx = (int)(i - (int64_t)yy * ow);
    uint32_t v0 = 0, v1 = 0, v2 = 0;
    if (!zeros) {
      if (d->need_v) {
        const int ymin = bounds[2 * yy] - yf, ymax = bounds[2 * yy + 1];
        const int32_t* k = kk + (int64_t)yy * ks;
        int32_t s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
        for (int y = 0; y < ymax; y++) {
          const uint8_t* p = src + ((int64_t)(y + ymin) * sw + xx) * 3;
          const int32_t c = k[y];
          s0 += p[0] * c;
          s1 += p[1] * c;
          s2 += p[2] * c;
        }
        v0 = clip8(s0);
        v1 = clip8(s1);
        v2 = clip8(s2);
      } else {
        const uint8_t* p = src + ((int64_t)yy * sw + xx) * 3;
        v0 = p[0];
        v1 = p[1];
        v2 = p[2];
      }
    }
    const int ox = fl ? ow - 1 - xx : xx;
    const int64_t pix = (int64_t)yy * ow + ox;
    if (f32) {
      float* b = of;
      if (hwc) {
        b[pix * 3] = lut[v0];
        b[pix * 3 + 1] = lut[v1];
        b[pix * 3 + 2] = lut[v2];
      } else {
        b[pix] = lut[v0];
        b[plane + pix] = lut[v1];
        b[2 * plane + pix] = lut[v2];
      }
    } else {
      uint8_t* b = o8;
      if (hwc) {
        b[pix * 3] = (uint8_t)v0;
        b[pix * 3 + 1] = (uint8_t)v1;
        b[pix * 3 + 2] = (uint8_t)v2;
      } else {
        b[pix] = (uint8_t)v0;
        b[plane + pix] = (uint8_t)v1;
        b[2 * plane + pix] = (uint8_t)v2;
      }
    }
  }
 }
}

// ------------------------------------------------------------------------------------------
// Host-side launchers (called by the engine; all asynchronous on `stream`).
// ------------------------------------------------------------------------------------------
hipError_t launch_color(int n, const ImgDesc* descs, uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s,
                        uint64_t rm) {
  if (!route_on(rm, kRtUnfused)) return hipSuccess;
  hipLaunchKernelGGL(k_color, dim3(64, n < 64 ? n : 64), dim3(256), 0, s, n, descs, scratch, routes, cap);
  return hipGetLastError();
}
hipError_t launch_cmyk(int rt, int n, const ImgDesc* descs, uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s,
                       uint64_t rm, uint64_t hint) {
  if (!route_on(rm, rt)) return hipSuccess;
  const dim3 grid(16, route_grid(hint, rt, n < 256 ? n : 256));
  if (rt == kRtProg4) hipLaunchKernelGGL(k_cmyk<kRtProg4>, grid, dim3(256), 0, s, descs, scratch, routes, cap);
  else hipLaunchKernelGGL(k_cmyk<kRtScans>, grid, dim3(256), 0, s, descs, scratch, routes, cap);
  return hipGetLastError();
}
hipError_t launch_coeffs(int n, ImgDesc* descs, const sdsj_op& op, uint8_t* scratch, hipStream_t s) {
  int mx = op.out_w > op.out_h ? op.out_w : op.out_h;
  hipLaunchKernelGGL(k_coeffs, dim3((mx + 255) / 256, n), dim3(256), 0, s, n, descs, op, scratch);
  return hipGetLastError();
}
hipError_t launch_hpass(int n, const ImgDesc* descs, const sdsj_op& op, uint8_t* scratch, const int32_t* routes, int cap,
                        hipStream_t s, uint64_t rm) {
  if (!route_on(rm, kRtUnfused)) return hipSuccess;
  hipLaunchKernelGGL(k_hpass, dim3(32, n < 64 ? n : 64), dim3(256), 0, s, n, descs, op, scratch, routes, cap);
  return hipGetLastError();
}
hipError_t launch_vpass(int n, const ImgDesc* descs, const sdsj_op& op, const uint8_t* scratch, const uint8_t* flip,
                        void* out, const int32_t* routes, int cap, const float* lut, hipStream_t s, uint64_t rm) {
  if (!route_on(rm, kRtUnfused)) return hipSuccess;
  hipLaunchKernelGGL(k_vpass, dim3(32, n < 64 ? n : 64), dim3(256), 0, s, n, descs, op, scratch, flip, out, routes, cap, lut);
  return hipGetLastError();
}

}  // namespace sdsj
