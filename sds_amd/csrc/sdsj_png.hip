// sdsj_png.hip -- gfx950 kernels of the opt-in PNG path (SDSJ_FORMAT_PNG) and sdsj_png_probe.
//
//   k_png_inflate   one wavefront per image: zlib / deflate over the IDAT chain into the image's
//                   scanline buffer (scratch, off_png), Adler-32 and the rows' filter bytes checked
//                   (sdsj_png_inflate_kernel.h, the one source of the three masks' inflate kernels)
//   k_png_unfilter one wavefront per image: filters 0-4 reversed, RGB rows written to off_rgb (gray
//                   replicated, palette looked up, alpha dropped), which k_hpass / k_vpass then read
// With SDSJ_FORMAT_PNG_EXT in the mask launch_png takes k_png_inflate_ext and adds k_png_unfilter_ext
// (sdsj_png_ext.hip) for what k_png_unfilter skips: Adam7 files and bit depths 1, 2, 4, 16.  With
// SDSJ_FORMAT_PNG_META it takes k_png_inflate_meta (sdsj_png_meta.hip), after k_png_meta has judged the
// compressed chunks and what follows the image data.
//
// Reference behaviour: PIL.Image.open(...).convert("RGB").  Every correctness and bounds decision is
// taken by the shared functions of sdsj_png.h (the same ones the sanitizer driver runs serially on
// the host); the kernels below only move bytes with 64 lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sdsj_common.h"
#include "sdsj_kernels.h"
#include "sdsj_png.h"
#include "sdsj_png_wave.h"

namespace sdsj {

namespace {

// k_png_inflate: the shared kernel with the filter-byte check over the rows of one plain image.
#define SDSJ_PNG_INFLATE_KERNEL k_png_inflate
#define SDSJ_PNG_INFLATE_PASSES 0
#define SDSJ_PNG_INFLATE_TAIL_JUDGED 0
#include "sdsj_png_inflate_kernel.h"


// Skewed wavefront over bands of 64 rows: lane j reconstructs row base + j and runs j pixels behind
// lane j - 1, so at every step its left pixel is its own previous result, its upper pixel the one
// lane j - 1 produced a step earlier (one lane shift of a packed dword) and its upper-left pixel the
// upper pixel it used a step earlier.  Lane 0 reads the band's upper row from the scanline buffer,
// where lane 63 of the previous band stored its reconstructed row in place.  All five filter types
// take this one path.
__global__ void __launch_bounds__(64) k_png_unfilter(const ImgDesc* __restrict__ descs, const uint8_t* __restrict__ blob,
                                                     const int64_t* __restrict__ offsets, uint8_t* scratch,
                                                     const int32_t* __restrict__ routes, int cap) {
  const int32_t* rl = route_list(routes, cap, kRtPng);
  const int lane = threadIdx.x;
  for (int li = blockIdx.x; li < routes[kRtPng]; li += gridDim.x) {
    const int img = rl[li];
    const ImgDesc* d = &descs[img];
    if (d->status != SDSJ_OK || !d->png || d->geo == kGeoZeros || !png_plain(d)) continue;  // (k_png_unfilter_ext's)
    const int w = d->width, bpp = d->png_bpp, ctype = d->png_ctype, plte_n = d->png_plte_n;
    const int rows = d->src_y1 < d->height ? d->src_y1 : d->height;  // later rows are not read
    const int64_t pitch = 1 + (int64_t)w * bpp;
    uint8_t* raw = scratch + d->off_png;
    uint8_t* rgb = scratch + d->off_rgb;
    const GlobalReader pal{blob + offsets[img] + d->png_plte_pos};
    const int x0 = d->src_x0, x1 = d->src_x0 + d->src_w, y0 = d->src_y0, sw = d->src_w;
    for (int base = 0; base < rows; base += 64) {
      const int y = base + lane;
      const bool rowok = y < rows;
      const int nrow = rows - base < 64 ? rows - base : 64;
      uint8_t* rowp = raw + (int64_t)(rowok ? y : 0) * pitch;
      const uint8_t* prevp = raw + (int64_t)(base > 0 ? base - 1 : 0) * pitch + 1;
      const int ft = rowok ? rowp[0] : 0;
      const bool keep = lane == 63 && base + 64 < rows;  // the next band's upper row
      uint32_t cur = 0, bprev = 0;
      const int steps = w + nrow - 1;
      for (int t = 0; t < steps; t++) {
        const int x = t - lane;
        const bool act = rowok && x >= 0 && x < w;
        uint32_t b = __shfl_up(cur, 1);
        if (act) {
          if (lane == 0) {
            b = 0;
            if (base > 0)
              for (int k = 0; k < bpp; k++) b |= (uint32_t)prevp[(int64_t)x * bpp + k] << (8 * k);
          }
          uint32_t px = 0;
          for (int k = 0; k < bpp; k++) px |= (uint32_t)rowp[1 + (int64_t)x * bpp + k] << (8 * k);
          const uint32_t rec = png_recon(ft, px, x > 0 ? cur : 0u, b, x > 0 ? bprev : 0u, bpp);
          cur = rec;
          bprev = b;
          if (keep)
            for (int k = 0; k < bpp; k++) rowp[1 + (int64_t)x * bpp + k] = (uint8_t)(rec >> (8 * k));
          if (y >= y0 && x >= x0 && x < x1) {
            const uint32_t c = png_rgb(ctype, rec, plte_n, pal);
            uint8_t* o = rgb + ((int64_t)(y - y0) * sw + (x - x0)) * 3;
            o[0] = (uint8_t)c;
            o[1] = (uint8_t)(c >> 8);
            o[2] = (uint8_t)(c >> 16);
          }
        }
      }
      wave_store_fence();
    }
  }
}

}  // namespace

hipError_t launch_png(int n, ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, const int32_t* lengths,
                      uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s, uint64_t rm, uint64_t hint,
                      hipEvent_t between, int formats) {
  if (!route_on(rm, kRtPng)) {
    if (between) (void)hipEventRecord(between, s);
    return hipSuccess;
  }
  const unsigned g = route_grid(hint, kRtPng, n);
  const bool ext = (formats & SDSJ_FORMAT_PNG_EXT) != 0;
  if (formats & SDSJ_FORMAT_PNG_META) launch_png_inflate_meta(g, descs, blob, offsets, lengths, scratch, routes, cap, s);
  else if (ext) launch_png_inflate_ext(g, descs, blob, offsets, lengths, scratch, routes, cap, s);
  else hipLaunchKernelGGL(k_png_inflate, dim3(g), dim3(64), 0, s, descs, blob, offsets, lengths, scratch, routes, cap);
  if (between) (void)hipEventRecord(between, s);
  hipLaunchKernelGGL(k_png_unfilter, dim3(g), dim3(64), 0, s, descs, blob, offsets, scratch, routes, cap);
  if (ext) launch_png_unfilter_ext(g, descs, blob, offsets, scratch, routes, cap, s);  // (counts under png_unfilter)
  return hipGetLastError();
}

}  // namespace sdsj

extern "C" int sdsj_png_probe(const uint8_t* png, size_t n, sdsj_png_info* out) {
  return sdsj_png_probe_formats(png, n, SDSJ_FORMAT_PNG, out);
}

extern "C" int sdsj_png_probe_formats(const uint8_t* png, size_t n, int formats, sdsj_png_info* out) {
  if (!png || !out || !(formats & SDSJ_FORMAT_PNG)) return SDSJ_EINVAL;
  memset(out, 0, sizeof(*out));
  sdsj::PngHdr h;
  const sdsj::GlobalReader rd{png};
  int st = sdsj::png_parse(rd, (int64_t)n, &h, formats);
  if (st == SDSJ_OK && (formats & SDSJ_FORMAT_PNG_META)) st = sdsj::host_png_meta(png, (int64_t)n, h.idat_pos, formats);
  out->width = h.width;
  out->height = h.height;
  out->bit_depth = h.bit_depth;
  out->color_type = h.ctype;
  out->interlace = h.interlace;
  out->supported = st == SDSJ_OK;
  return st;
}
