// sdsj_png_inflate_kernel.h -- the one definition of the PNG inflate kernel: one wavefront per image, zlib /
// deflate over the IDAT chain into the image's scanline buffer (scratch, off_png), Adler-32 and the rows'
// filter bytes checked.
//
// No include guard: included exactly once per translation unit, inside `namespace sdsj { namespace {`,
// after sdsj_png.h and sdsj_png_wave.h, with three macros defined in front (all undefined again at the end):
//   SDSJ_PNG_INFLATE_KERNEL       the kernel's name
//   SDSJ_PNG_INFLATE_PASSES       0: the filter bytes of the rows of one plain image
//                                 1: those of the rows of every pass (wave_filter_bytes_bad; only the kernels
//                                    built with 1 call it: engines with the base mask keep the kernel without the walk)
//   SDSJ_PNG_INFLATE_TAIL_JUDGED  1: png_tail_ok's SDSJ_UNSUPPORTED does not count, k_png_meta has judged the tail
//                                    under the mask
// sdsj_png.hip (0, 0), sdsj_png_ext.hip (1, 0) and sdsj_png_meta.hip (1, 1) each build their kernel from it.  The
// preprocessor and separate translation units, not a template body or one translation unit: those compile
// k_png_inflate to other machine code than the written-out kernel had ("PNG"), this form to the same.
#if !defined(SDSJ_PNG_INFLATE_KERNEL) || !defined(SDSJ_PNG_INFLATE_PASSES) || !defined(SDSJ_PNG_INFLATE_TAIL_JUDGED)
#error "define SDSJ_PNG_INFLATE_KERNEL, SDSJ_PNG_INFLATE_PASSES and SDSJ_PNG_INFLATE_TAIL_JUDGED before including"
#endif

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) SDSJ_PNG_INFLATE_KERNEL(ImgDesc* __restrict__ descs, const uint8_t* __restrict__ blob,
                                                   const int64_t* __restrict__ offsets,
                                                   const int32_t* __restrict__ lengths, uint8_t* scratch,
                                                   const int32_t* __restrict__ routes, int cap) {
  __shared__ InfTables T;
  __shared__ uint8_t win[kWin];
  const int32_t* rl = route_list(routes, cap, kRtPng);
  const int lane = threadIdx.x;
  for (int li = blockIdx.x; li < routes[kRtPng]; li += gridDim.x) {
    const int img = rl[li];
    ImgDesc* d = &descs[img];
    if (d->status != SDSJ_OK || !d->png) continue;
    const WindowReader rd{blob + offsets[img], (int64_t)lengths[img], win, lane, -(int64_t)4 * kWin};
    const int64_t expect = d->png_raw;
    uint8_t* out = scratch + d->off_png;
    PngBits<WindowReader> br;
    png_bits_init(br, rd, rd.n, d->png_idat_pos);
    WaveSink sink{out, 0, 0, 0u, lane};
    uint32_t want = 0;
    int st = png_inflate(br, &T, sink, expect, &want);
#if SDSJ_PNG_INFLATE_TAIL_JUDGED
    if (st == SDSJ_UNSUPPORTED) st = SDSJ_OK;  // png_tail_ok's strict answer
#endif
    sink.flush();
    wave_store_fence();
    if (st == SDSJ_OK) {
      if (wave_adler(out, expect, lane) != want) st = SDSJ_CORRUPT;
      // a filter type above 4 is an error in ZipDecode.c: the first byte of every row (of every pass)
#if SDSJ_PNG_INFLATE_PASSES
      if (__ballot(wave_filter_bytes_bad(out, d->width, d->height, d->png_ctype, png_ihdr(d), lane))) st = SDSJ_CORRUPT;
#else
      const int64_t pitch = 1 + (int64_t)d->width * d->png_bpp;
      bool bad = false;
      for (int y = lane; y < d->height; y += 64) bad |= out[(int64_t)y * pitch] > 4;
      if (__ballot(bad)) st = SDSJ_CORRUPT;
#endif
    }
    __syncthreads();  // T is rebuilt by the next image
    if (st != SDSJ_OK && lane == 0) d->status = st;
  }
}

#undef SDSJ_PNG_INFLATE_KERNEL
#undef SDSJ_PNG_INFLATE_PASSES
#undef SDSJ_PNG_INFLATE_TAIL_JUDGED
