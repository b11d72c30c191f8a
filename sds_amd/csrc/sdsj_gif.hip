// sdsj_gif.hip -- gfx950 kernels of the opt-in GIF path (SDSJ_FORMAT_GIF) and sdsj_gif_probe.
//
//   k_gif_lzw  one wavefront per image: LZW over the data sub-blocks into the image's index buffer
//              (scratch, off_png: the frame's fw x fh bytes in stream order)
//   k_gif_rgb  RGB rows [src_y0, src_y1) x [src_x0, src_x0 + src_w) written to off_rgb (frame rows
//              de-interlaced, the fill index outside the frame, the colour table read from the sample's
//              bytes), which k_hpass / k_vpass then read
// launch_gif is called by the engine only when its mask has the bit.
//
// Reference behaviour: PIL.Image.open(...).convert("RGB"), first frame.  Every correctness and bounds
// decision is taken by the shared functions of sdsj_gif.h (the same ones the sanitizer driver runs
// serially on the host); the kernels below only move bytes with 64 lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sdsj_common.h"
#include "sdsj_gif.h"
#include "sdsj_kernels.h"
#include "sdsj_png_wave.h"

namespace sdsj {

namespace {

// The decode is wave-uniform, like the inflate kernel's: every lane reads the same codes through the LDS
// window, holds the same state and writes the same table entries; literals are batched into one store of
// up to 64 bytes and a string is copied from the earlier output by all lanes (WaveSink: a fence, then 64
// bytes per step).  LDS per wave: the table's 24 KiB (GifTable) and the 1 KiB window, so six waves share a
// CU's 160 KiB.  (Keeping strings of up to four bytes in the table entries, so that they never read the
// output back, measured no faster -- DESIGN.md, "GIF": the wave-uniform chain per code is the bound.)
__global__ void __launch_bounds__(64) k_gif_lzw(ImgDesc* __restrict__ descs, const uint8_t* __restrict__ blob,
                                                const int64_t* __restrict__ offsets, const int32_t* __restrict__ lengths,
                                                uint8_t* scratch, const int32_t* __restrict__ routes, int cap) {
  __shared__ GifTable T;
  __shared__ uint8_t win[kWin];
  const int32_t* rl = route_list(routes, cap, kRtGif);
  const int lane = threadIdx.x;
  for (int li = blockIdx.x; li < routes[kRtGif]; li += gridDim.x) {
    const int img = rl[li];
    ImgDesc* d = &descs[img];
    if (d->status != SDSJ_OK || d->png != kGifSample) continue;
    const GifView v = gif_view(*d);
    const int64_t expect = (int64_t)v.fw * v.fh;
    int st = SDSJ_CORRUPT;
    if (expect > 0 && expect <= d->png_raw) {  // (gif_parse: the frame lies inside the screen)
      const WindowReader rd{blob + offsets[img], (int64_t)lengths[img], win, lane, -(int64_t)4 * kWin};
      GifBits<WindowReader> br;
      gif_bits_init(br, rd, rd.n, d->png_idat_pos);
      WaveSink sink{scratch + d->off_png, 0, 0, 0u, lane};
      st = gif_lzw(br, &T, sink, expect, d->png_depth_lace & 255);
      sink.flush();
    }
    __syncthreads();  // T and the window are the next image's
    if (st != SDSJ_OK && lane == 0) d->status = st;
  }
}

// One workgroup per (image, row slice); a thread per pixel of the rows and columns the resample needs.
constexpr int kGifRgbThreads = 256, kGifRgbSlices = 8;
__global__ void __launch_bounds__(kGifRgbThreads) k_gif_rgb(const ImgDesc* __restrict__ descs, const uint8_t* __restrict__ blob,
                                                            const int64_t* __restrict__ offsets, uint8_t* scratch,
                                                            const int32_t* __restrict__ routes, int cap) {
  const int32_t* rl = route_list(routes, cap, kRtGif);
  for (int li = blockIdx.x; li < routes[kRtGif]; li += gridDim.x) {
    const int img = rl[li];
    const ImgDesc* d = &descs[img];
    if (d->status != SDSJ_OK || d->png != kGifSample || d->geo == kGeoZeros) continue;
    const GifView v = gif_view(*d);
    const int y0 = d->src_y0 < 0 ? 0 : d->src_y0, y1 = d->src_y1 < d->height ? d->src_y1 : d->height;
    const int x0 = d->src_x0, sw = d->src_w;
    if (x0 < 0 || sw <= 0 || x0 + sw > d->width || y1 <= y0) continue;
    const GlobalReader idx{scratch + d->off_png}, pal{blob + offsets[img] + d->png_plte_pos};
    uint8_t* rgb = scratch + d->off_rgb;
    const int rows = y1 - y0, per = (rows + kGifRgbSlices - 1) / kGifRgbSlices;
    const int r0 = blockIdx.y * per, r1 = r0 + per < rows ? r0 + per : rows;
    const int64_t p0 = (int64_t)r0 * sw, p1 = (int64_t)r1 * sw;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += kGifRgbThreads) {
      const int ry = (int)(p / sw), rx = (int)(p - (int64_t)ry * sw);
      const uint32_t c = gif_rgb(gif_index_at(v, idx, x0 + rx, y0 + ry), v.table_n, pal);
      uint8_t* o = rgb + ((int64_t)(y0 + ry - d->src_y0) * sw + rx) * 3;
      o[0] = (uint8_t)c;
      o[1] = (uint8_t)(c >> 8);
      o[2] = (uint8_t)(c >> 16);
    }
  }
}

}  // namespace

hipError_t launch_gif(int n, ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, const int32_t* lengths,
                      uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s, uint64_t rm, uint64_t hint) {
  if (!route_on(rm, kRtGif) || n <= 0) return hipSuccess;
  const unsigned g = route_grid(hint, kRtGif, n);
  hipLaunchKernelGGL(k_gif_lzw, dim3(g), dim3(64), 0, s, descs, blob, offsets, lengths, scratch, routes, cap);
  hipLaunchKernelGGL(k_gif_rgb, dim3(g, kGifRgbSlices), dim3(kGifRgbThreads), 0, s, descs, blob, offsets, scratch, routes, cap);
  return hipGetLastError();
}

}  // namespace sdsj

extern "C" int sdsj_gif_probe(const uint8_t* gif, size_t n, sdsj_gif_info* out) {
  if (!gif || !out) return SDSJ_EINVAL;
  memset(out, 0, sizeof(*out));
  sdsj::GifHdr h;
  const sdsj::GlobalReader rd{gif};
  const int st = sdsj::gif_parse(rd, (int64_t)n, &h);
  out->width = h.width;
  out->height = h.height;
  out->frame_x = h.fx;
  out->frame_y = h.fy;
  out->frame_w = h.fw;
  out->frame_h = h.fh;
  out->interlace = h.interlace;
  out->table_entries = h.table_n;
  out->min_code_size = h.min_code;
  out->supported = st == SDSJ_OK;
  return st;
}
