// sdsj_png_ext.hip -- gfx950 kernels of the wider PNG subset (SDSJ_FORMAT_PNG_EXT: Adam7 interlace, bit
// depths 1, 2, 4, 16), launched by launch_png (sdsj_png.hip) only when the engine's mask has the bit.
//
//   k_png_inflate_ext   k_png_inflate with the filter-byte check walking the rows of every pass
//                       (sdsj_png_inflate_kernel.h)
//   k_png_unfilter_ext  one wavefront per (image, pass) for what k_png_unfilter skips
//
// A translation unit of its own: the base subset's kernels are compiled exactly as without it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdsj_common.h"
#include "sdsj_kernels.h"
#include "sdsj_png.h"
#include "sdsj_png_wave.h"

namespace sdsj {

namespace {

// k_png_inflate_ext: the shared kernel with the filter-byte check over the rows of every pass.
#define SDSJ_PNG_INFLATE_KERNEL k_png_inflate_ext
#define SDSJ_PNG_INFLATE_PASSES 1
#define SDSJ_PNG_INFLATE_TAIL_JUDGED 0
#include "sdsj_png_inflate_kernel.h"


// What k_png_unfilter skips, one wavefront per (image, pass): the passes of an Adam7 image are
// independent once inflated.  Within a pass the same skewed wavefront over bands of 64 pass rows, over
// filter units (1 to 8 bytes, packed in 64 bits) instead of pixels: a unit is one pixel from depth 8 on
// and 8 / 4 / 2 pixels of one byte below.  The store unpacks the unit's pixels (png_rgb_ext), maps pass
// coordinates to image coordinates (x = xs + px * dx, y = ys + py * dy) and applies the crop to those;
// pass rows whose image row is at or beyond src_y1 are not reconstructed.
__global__ void __launch_bounds__(64) k_png_unfilter_ext(const ImgDesc* __restrict__ descs, const uint8_t* __restrict__ blob,
                                                         const int64_t* __restrict__ offsets, uint8_t* scratch,
                                                         const int32_t* __restrict__ routes, int cap) {
  const int32_t* rl = route_list(routes, cap, kRtPng);
  const int lane = threadIdx.x;
  const int items = routes[kRtPng] * 7;
  for (int it = blockIdx.x; it < items; it += gridDim.x) {
    const int img = rl[it / 7], slot = it % 7;
    const ImgDesc* d = &descs[img];
    if (d->status != SDSJ_OK || !d->png || d->geo == kGeoZeros) continue;
    const PngIhdr ih = png_ihdr(d);
    if (png_plain(d) || (!ih.interlace && slot > 0)) continue;
    PngPass ps;
    if (!png_pass_at(d->width, d->height, d->png_ctype, ih.depth, ih.interlace, slot, &ps)) continue;
    const int depth = ih.depth, unit = d->png_bpp, ctype = d->png_ctype, plte_n = d->png_plte_n;
    const int ppu = depth < 8 ? 8 / depth : 1;  // pixels per unit
    const int nu = (int)(ps.rowbytes / unit);   // units per row
    // pass rows whose image row lies before src_y1 (and inside the image: ps.h)
    int rows = d->src_y1 > ps.ys ? (d->src_y1 - ps.ys + ps.dy - 1) / ps.dy : 0;
    rows = rows < ps.h ? rows : ps.h;
    const int64_t pitch = 1 + ps.rowbytes;
    uint8_t* raw = scratch + d->off_png + ps.off;
    uint8_t* rgb = scratch + d->off_rgb;
    const GlobalReader pal{blob + offsets[img] + d->png_plte_pos};
    const int x0 = d->src_x0, x1 = d->src_x0 + d->src_w, y0 = d->src_y0, sw = d->src_w;
    for (int base = 0; base < rows; base += 64) {
      const int py = base + lane;
      const bool rowok = py < rows;
      const int nrow = rows - base < 64 ? rows - base : 64;
      uint8_t* rowp = raw + (int64_t)(rowok ? py : 0) * pitch;
      const uint8_t* prevp = raw + (int64_t)(base > 0 ? base - 1 : 0) * pitch + 1;
      const int ft = rowok ? rowp[0] : 0;
      const bool keep = lane == 63 && base + 64 < rows;  // the next band's upper row
      const int y = ps.ys + py * ps.dy;
      const bool yin = y >= y0;  // (y < src_y1 by the choice of rows)
      uint64_t cur = 0, bprev = 0;
      const int steps = nu + nrow - 1;
      for (int t = 0; t < steps; t++) {
        const int u = t - lane;
        const bool act = rowok && u >= 0 && u < nu;
        uint64_t b = __shfl_up(cur, 1);
        if (act) {
          if (lane == 0) {
            b = 0;
            if (base > 0)
              for (int k = 0; k < unit; k++) b |= (uint64_t)prevp[(int64_t)u * unit + k] << (8 * k);
          }
          uint64_t px = 0;
          for (int k = 0; k < unit; k++) px |= (uint64_t)rowp[1 + (int64_t)u * unit + k] << (8 * k);
          const uint64_t rec = png_recon(ft, px, u > 0 ? cur : (uint64_t)0, b, u > 0 ? bprev : (uint64_t)0, unit);
          cur = rec;
          bprev = b;
          if (keep)
            for (int k = 0; k < unit; k++) rowp[1 + (int64_t)u * unit + k] = (uint8_t)(rec >> (8 * k));
          if (yin) {
            for (int k = 0; k < ppu; k++) {
              const int pxl = u * ppu + k;  // pixel of the pass row; those beyond its width are padding bits
              const int x = ps.xs + pxl * ps.dx;
              if (pxl < ps.w && x >= x0 && x < x1) {
                const uint32_t c = png_rgb_ext(ctype, depth, rec, k, plte_n, pal);
                uint8_t* o = rgb + ((int64_t)(y - y0) * sw + (x - x0)) * 3;
                o[0] = (uint8_t)c;
                o[1] = (uint8_t)(c >> 8);
                o[2] = (uint8_t)(c >> 16);
              }
            }
          }
        }
      }
      wave_store_fence();
    }
  }
}

}  // namespace

void launch_png_inflate_ext(unsigned g, ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, const int32_t* lengths,
                            uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s) {
  hipLaunchKernelGGL(k_png_inflate_ext, dim3(g), dim3(64), 0, s, descs, blob, offsets, lengths, scratch, routes, cap);
}

void launch_png_unfilter_ext(unsigned g, const ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, uint8_t* scratch,
                             const int32_t* routes, int cap, hipStream_t s) {
  // (image, pass) work items
  hipLaunchKernelGGL(k_png_unfilter_ext, dim3(7 * g), dim3(64), 0, s, descs, blob, offsets, scratch, routes, cap);
}

}  // namespace sdsj
