// sdsj_png_meta.hip -- gfx950 kernels of SDSJ_FORMAT_PNG_META (iCCP, zTXt, iTXt and chunks after the image
// data), launched only when the engine's mask has the bit.
//
//   k_png_meta          one wavefront per sample, between k_parse and k_plan: png_meta_check (sdsj_png.h) --
//                       the size rule over the compressed chunks (a count-only inflate: no output, no
//                       window), the text budget, the walk over the chunks after the IDAT run.  A sample it
//                       refuses turns SDSJ_UNSUPPORTED before scratch is planned for it, so the statuses and
//                       the scratch need are those of host planning (host_png_meta runs the same function).
//   k_png_inflate_meta  k_png_inflate_ext that ignores the strict answer of png_tail_ok, which k_png_meta has
//                       replaced; it serves the mask with and without SDSJ_FORMAT_PNG_EXT (the walk over
//                       the passes of a plain image is the check of its rows) (sdsj_png_inflate_kernel.h).
//
// A translation unit of its own: the kernels of the other masks are compiled exactly as without it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdsj_common.h"
#include "sdsj_kernels.h"
#include "sdsj_png.h"
#include "sdsj_png_wave.h"

namespace sdsj {

namespace {

// k_png_inflate_meta: k_png_inflate_ext for which png_tail_ok's refusal does not count: the tail is k_png_meta's.
#define SDSJ_PNG_INFLATE_KERNEL k_png_inflate_meta
#define SDSJ_PNG_INFLATE_PASSES 1
#define SDSJ_PNG_INFLATE_TAIL_JUDGED 1
#include "sdsj_png_inflate_kernel.h"

// The chunk bytes come through the LDS window, the tables of the count-only inflate sit in LDS, and the
// walk is wave-uniform: every lane holds the same state and takes the same branches (the window's
// barriers are met by all 64).  k_parse has checked that the sample lies inside the blob and that
// every chunk before png_idat_pos lies inside the sample; the walk reads no byte outside [0, length).
//
// Three waves per SIMD, 168 VGPRs like the inflate kernels (45 spilled, 88 bytes of scratch; the kernel reads a few
// KB per sample): a lane of a batch runs this kernel while the lanes before it inflate, two waves of 168 VGPRs on
// every SIMD, and at the 207 VGPRs the compiler takes unasked it found no room beside them -- the lanes then ran one
// after the other, and a batch of 4,096 plain 640x480 files took 740 instead of 690 ms.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) k_png_meta(int n, ImgDesc* __restrict__ descs, const uint8_t* __restrict__ blob,
                                                 const int64_t* __restrict__ offsets, const int32_t* __restrict__ lengths,
                                                 int formats) {
  __shared__ InfTables T;
  __shared__ uint8_t win[kWin];
  const int img = blockIdx.x, lane = threadIdx.x;
  if (img >= n) return;
  ImgDesc* d = &descs[img];
  if (d->status != SDSJ_OK || d->png != 1) return;  // (2: a GIF sample)
  const WindowReader rd{blob + offsets[img], (int64_t)lengths[img], win, lane, -(int64_t)4 * kWin};
  const int st = png_meta_check(rd, rd.n, d->png_idat_pos, formats, &T);
  if (st != SDSJ_OK && lane == 0) d->status = st;
}

}  // namespace

hipError_t launch_png_meta(int n, ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, const int32_t* lengths,
                           hipStream_t s, int formats) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_png_meta, dim3(n), dim3(64), 0, s, n, descs, blob, offsets, lengths, formats);
  return hipGetLastError();
}

void launch_png_inflate_meta(unsigned g, ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, const int32_t* lengths,
                             uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s) {
  hipLaunchKernelGGL(k_png_inflate_meta, dim3(g), dim3(64), 0, s, descs, blob, offsets, lengths, scratch, routes, cap);
}

int host_png_meta(const uint8_t* png, int64_t n, int64_t idat_pos, int formats) {
  static thread_local InfTables T;
  return png_meta_check(GlobalReader{png}, n, idat_pos, formats, &T);
}

}  // namespace sdsj
