// sdsj_tiff.hip -- gfx950 kernels of the opt-in TIFF path (SDSJ_FORMAT_TIFF) and sdsj_tiff_probe.
//
// A TIFF's strips are compressed independently, so the strip kernels spend one wavefront per (sample, strip):
// grid x walks the route list as the other kernels do, grid y walks the sample's strips with a stride loop,
// and each wavefront writes its strip's rows straight to their place at off_png (height x width x samples
// bytes).  The compressions are kept apart, each kernel skipping the samples of the other kinds, so a
// wavefront's LDS is one codec's tables plus the 1 KiB window:
//   k_tiff_copy     uncompressed strips (the sample's wavefronts share every strip's bytes) and PackBits (a uniform control walk through the
//                   window, all lanes moving each run)
//   k_tiff_lzw      LZW, wave-uniform like k_gif_lzw: the table in LDS, literals batched, strings copied from
//                   the strip's earlier output by all lanes
//   k_tiff_inflate  Deflate: the inflate of the PNG path over one contiguous range, Adler-32 checked
// Every strip is decoded, also those outside the crop: the status depends on all of them.  A failing strip
// lowers the sample's status with atomicMin (several wavefronts write that field).
//   k_tiff_rgb      rows [src_y0, src_y1) x [src_x0, src_x0 + src_w) as packed RGB at off_rgb: predictor 2
//                   undone by a wave prefix sum along each row per sample (modulo 256), then inversion,
//                   ColorMap lookup (read from the sample's bytes), extra-sample drop or CMYK -> RGB; k_hpass /
//                   k_vpass read from there
// launch_tiff is called by the engine only when its mask has the bit.
//
// Reference behaviour: PIL.Image.open(...).convert("RGB").  Every correctness and bounds decision is taken by
// the shared functions of sdsj_tiff.h (the same ones the sanitizer driver runs serially on the host).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sdsj_common.h"
#include "sdsj_kernels.h"
#include "sdsj_png_wave.h"
#include "sdsj_tiff.h"

namespace sdsj {

namespace {

constexpr int kTiffStripY = 16;  // grid y of the strip kernels (Pillow / libtiff write 5 to 20 strips for 640 x 480)

// The strip a wavefront decodes, or false: the descriptor's view, the strip's range in the sample and its place
// in the decoded samples at off_png.
struct TiffJob {
  TiffStrip sp;
  uint8_t* out;
};
__device__ __forceinline__ bool tiff_job(const ImgDesc* d, const TiffView& v, const uint8_t* in, int64_t n, uint8_t* scratch,
                                         int s, TiffJob* j) {
  const GlobalReader gr{in};
  if (!tiff_strip(gr, n, v, d->width, d->height, s, &j->sp)) return false;
  const int64_t at = (int64_t)j->sp.row0 * d->width * v.spp;
  if (j->sp.expect < 1 || at + j->sp.expect > d->png_raw) return false;  // (cannot fail: row0 + rows <= height)
  j->out = scratch + d->off_png + at;
  return true;
}

// The sample's status as the strip kernels read it: other wavefronts of the same sample may lower it meanwhile
// (tiff_lower), so the load is an atomic one.  Whichever value it sees is fine: a strip skipped because the status
// is already lowered belongs to a sample that fails anyway, and k_tiff_rgb reads it in a later kernel.
__device__ __forceinline__ int tiff_status(const ImgDesc* d) { return __atomic_load_n(&d->status, __ATOMIC_RELAXED); }

__device__ __forceinline__ void tiff_lower(ImgDesc* d, int st, int lane) {
  if (st != SDSJ_OK && lane == 0) atomicMin(&d->status, st);
}

// The PackBits sink of a wavefront: a run is moved by all lanes.  tiff_packbits has validated every position.
struct WaveRunSink {
  uint8_t* out;
  const uint8_t* in;
  int64_t pos;
  int lane;
  __device__ __forceinline__ void copy(int64_t src, int k) {
    for (int i = lane; i < k; i += 64) out[pos + i] = in[src + i];
    pos += k;
  }
  __device__ __forceinline__ void fill(int b, int k) {
    for (int i = lane; i < k; i += 64) out[pos + i] = (uint8_t)b;
    pos += k;
  }
};

__global__ void __launch_bounds__(64) k_tiff_copy(ImgDesc* __restrict__ descs, const uint8_t* __restrict__ blob,
                                                  const int64_t* __restrict__ offsets, const int32_t* __restrict__ lengths,
                                                  uint8_t* scratch, const int32_t* __restrict__ routes, int cap) {
  __shared__ uint8_t win[kWin];
  const int32_t* rl = route_list(routes, cap, kRtTiff);
  const int lane = threadIdx.x;
  for (int li = blockIdx.x; li < routes[kRtTiff]; li += gridDim.x) {
    const int img = rl[li];
    ImgDesc* d = &descs[img];
    if (tiff_status(d) != SDSJ_OK || d->png != kTiffSample) continue;
    const TiffView v = tiff_view(*d);
    if (v.codec != kTiffNone && v.codec != kTiffPackBits) continue;
    const uint8_t* in = blob + offsets[img];
    const int64_t n = (int64_t)lengths[img];
    if (v.codec == kTiffNone) {
      // Nothing is serial in an uncompressed strip, and Pillow writes such a file as one strip: every wavefront of
      // the sample's grid column walks all strips and copies its share of each, bytes [expect * y / Y, expect *
      // (y + 1) / Y) (tiff_strip: the strip's count covers its rows; expect <= 2^30).
      for (int s = 0; s < v.nstrips; s++) {
        TiffJob j;
        int st = SDSJ_CORRUPT;
        if (tiff_job(d, v, in, n, scratch, s, &j)) {
          const int64_t i0 = j.sp.expect * blockIdx.y / gridDim.y, i1 = j.sp.expect * (blockIdx.y + 1) / gridDim.y;
          for (int64_t i = i0 + lane; i < i1; i += 64) j.out[i] = in[j.sp.pos + i];
          st = SDSJ_OK;
        }
        tiff_lower(d, st, lane);
      }
      continue;
    }
    for (int s = blockIdx.y; s < v.nstrips; s += gridDim.y) {
      TiffJob j;
      int st = SDSJ_CORRUPT;
      if (tiff_job(d, v, in, n, scratch, s, &j)) {
        const WindowReader rd{in, n, win, lane, -(int64_t)4 * kWin};
        WaveRunSink sink{j.out, in, 0, lane};
        st = tiff_packbits(rd, j.sp.pos, j.sp.pos + j.sp.len, sink, j.sp.expect);
      }
      __syncthreads();  // the window is the next strip's
      tiff_lower(d, st, lane);
    }
  }
}

__global__ void __launch_bounds__(64) k_tiff_lzw(ImgDesc* __restrict__ descs, const uint8_t* __restrict__ blob,
                                                 const int64_t* __restrict__ offsets, const int32_t* __restrict__ lengths,
                                                 uint8_t* scratch, const int32_t* __restrict__ routes, int cap) {
  __shared__ GifTable T;
  __shared__ uint8_t win[kWin];
  const int32_t* rl = route_list(routes, cap, kRtTiff);
  const int lane = threadIdx.x;
  for (int li = blockIdx.x; li < routes[kRtTiff]; li += gridDim.x) {
    const int img = rl[li];
    ImgDesc* d = &descs[img];
    if (tiff_status(d) != SDSJ_OK || d->png != kTiffSample) continue;
    const TiffView v = tiff_view(*d);
    if (v.codec != kTiffLzw) continue;
    const uint8_t* in = blob + offsets[img];
    const int64_t n = (int64_t)lengths[img];
    for (int s = blockIdx.y; s < v.nstrips; s += gridDim.y) {
      TiffJob j;
      int st = SDSJ_CORRUPT;
      if (tiff_job(d, v, in, n, scratch, s, &j)) {
        const WindowReader rd{in, n, win, lane, -(int64_t)4 * kWin};
        TiffBits<WindowReader> br;
        tiff_bits_init(br, rd, j.sp.pos, j.sp.pos + j.sp.len);
        WaveSink sink{j.out, 0, 0, 0u, lane};
        st = tiff_lzw(br, &T, sink, j.sp.expect);
        sink.flush();
      }
      __syncthreads();  // T and the window are the next strip's
      tiff_lower(d, st, lane);
    }
  }
}

// Adler-32 of p[0, n) by one wave, p at any alignment: lane l sums the bytes of its segment of the dwords around
// p (s1 and s2 from zero), the segments are then chained in lane order (wave_adler wants an aligned p; a strip
// starts at its first row's place).
__device__ uint32_t tiff_wave_adler(const uint8_t* p, int64_t n, int lane) {
  const int64_t a = (int64_t)(reinterpret_cast<uintptr_t>(p) & 3);
  const uint8_t* q = p - a;  // aligned; the bytes are q[a, a + n)
  const int64_t seg = align_up((n + a + 63) / 64, 4);
  int64_t j0 = (int64_t)lane * seg, j1 = j0 + seg;
  j0 = j0 < a ? a : j0;
  j0 = j0 < n + a ? j0 : n + a;
  j1 = j1 < n + a ? j1 : n + a;
  j1 = j1 < j0 ? j0 : j1;
  uint64_t s1 = 0, s2 = 0;
  int64_t j = j0;
  for (; j < j1 && (j & 3); j++) {
    s1 += q[j];
    s2 += s1;
  }
  for (; j + 4 <= j1; j += 4) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(q + j);
    s1 += w & 255;
    s2 += s1;
    s1 += (w >> 8) & 255;
    s2 += s1;
    s1 += (w >> 16) & 255;
    s2 += s1;
    s1 += w >> 24;
    s2 += s1;
  }
  for (; j < j1; j++) {
    s1 += q[j];
    s2 += s1;
  }
  const uint32_t al = (uint32_t)(s1 % kAdlerMod), bl = (uint32_t)(s2 % kAdlerMod), ll = (uint32_t)((j1 - j0) % kAdlerMod);
  uint32_t S1 = 1, S2 = 0;
  for (int l = 0; l < 64; l++) {
    const uint32_t xa = __shfl(al, l), xb = __shfl(bl, l), xl = __shfl(ll, l);
    S2 = (uint32_t)((S2 + (uint64_t)S1 * xl + xb) % kAdlerMod);
    S1 = (S1 + xa) % kAdlerMod;
  }
  return (S2 << 16) | S1;
}

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3)))
k_tiff_inflate(ImgDesc* __restrict__ descs, const uint8_t* __restrict__ blob, const int64_t* __restrict__ offsets,
               const int32_t* __restrict__ lengths, uint8_t* scratch, const int32_t* __restrict__ routes, int cap) {
  __shared__ InfTables T;
  __shared__ uint8_t win[kWin];
  const int32_t* rl = route_list(routes, cap, kRtTiff);
  const int lane = threadIdx.x;
  for (int li = blockIdx.x; li < routes[kRtTiff]; li += gridDim.x) {
    const int img = rl[li];
    ImgDesc* d = &descs[img];
    if (tiff_status(d) != SDSJ_OK || d->png != kTiffSample) continue;
    const TiffView v = tiff_view(*d);
    if (v.codec != kTiffDeflate) continue;
    const uint8_t* in = blob + offsets[img];
    const int64_t n = (int64_t)lengths[img];
    for (int s = blockIdx.y; s < v.nstrips; s += gridDim.y) {
      TiffJob j;
      int st = SDSJ_CORRUPT;
      if (tiff_job(d, v, in, n, scratch, s, &j)) {
        const WindowReader rd{in, n, win, lane, -(int64_t)4 * kWin};
        PngBits<WindowReader> br;
        png_bits_span(br, rd, n, j.sp.pos, j.sp.pos + j.sp.len);
        WaveSink sink{j.out, 0, 0, 0u, lane};
        uint32_t want = 0;
        st = tiff_inflate(br, &T, sink, j.sp.expect, &want);
        sink.flush();
        wave_store_fence();
        if (st == SDSJ_OK && tiff_wave_adler(j.out, j.sp.expect, lane) != want) st = SDSJ_CORRUPT;
      }
      __syncthreads();  // T and the window are the next strip's
      tiff_lower(d, st, lane);
    }
  }
}

// One workgroup per (image, row slice), a wavefront per row: lane l takes pixel 64 k + l of the row's k-th chunk.
// With predictor 2 the chunks start at the row's first pixel and each is scanned (inclusive prefix sum per
// sample, modulo 256) on top of the chunks before it; without, they start at the crop.
constexpr int kTiffRgbThreads = 256, kTiffRgbSlices = 8;
__global__ void __launch_bounds__(kTiffRgbThreads) k_tiff_rgb(const ImgDesc* __restrict__ descs, const uint8_t* __restrict__ blob,
                                                              const int64_t* __restrict__ offsets, uint8_t* scratch, const int32_t* __restrict__ routes, int cap) {
  const int32_t* rl = route_list(routes, cap, kRtTiff);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int li = blockIdx.x; li < routes[kRtTiff]; li += gridDim.x) {
    const int img = rl[li];
    const ImgDesc* d = &descs[img];
    if (d->status != SDSJ_OK || d->png != kTiffSample || d->geo == kGeoZeros) continue;
    const TiffView v = tiff_view(*d);
    const int w = d->width, spp = v.spp;
    const int y0 = d->src_y0 < 0 ? 0 : d->src_y0, y1 = d->src_y1 < d->height ? d->src_y1 : d->height;
    const int x0 = d->src_x0, sw = d->src_w;
    if (x0 < 0 || sw <= 0 || x0 + sw > w || y1 <= y0 || spp < 1 || spp > 4) continue;
    const uint8_t* raw = scratch + d->off_png;
    const GlobalReader cmap{blob + offsets[img] + d->png_plte_pos};
    uint8_t* rgb = scratch + d->off_rgb;
    const int rows = y1 - y0, per = (rows + kTiffRgbSlices - 1) / kTiffRgbSlices;
    const int r0 = blockIdx.y * per, r1 = r0 + per < rows ? r0 + per : rows;
    const bool pred = v.predictor == 2;
    for (int ry = r0 + wave; ry < r1; ry += kTiffRgbThreads / 64) {
      const int y = y0 + ry;
      const uint8_t* row = raw + (int64_t)y * w * spp;
      uint8_t* o = rgb + (int64_t)(y - d->src_y0) * sw * 3;
      uint32_t carry = 0;
      for (int xb = pred ? 0 : (x0 & ~63); xb < x0 + sw; xb += 64) {
        const int x = xb + lane;
        uint32_t px = 0;
        if (x < w) {
          const uint8_t* s = row + (int64_t)x * spp;
          px = s[0];
          if (spp > 1) px |= (uint32_t)s[1] << 8;
          if (spp > 2) px |= (uint32_t)s[2] << 16;
          if (spp > 3) px |= (uint32_t)s[3] << 24;
        }
        if (pred) {
          for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(px, off);
            if (lane >= off) px = tiff_unpredict(px, t);
          }
          px = tiff_unpredict(px, carry);
          carry = __shfl(px, 63);
        }
        if (x >= x0 && x < x0 + sw) {
          const uint32_t c = tiff_rgb(px, v.photo, v.be, cmap);
          uint8_t* q = o + (int64_t)(x - x0) * 3;
          q[0] = (uint8_t)c;
          q[1] = (uint8_t)(c >> 8);
          q[2] = (uint8_t)(c >> 16);
        }
      }
    }
  }
}

}  // namespace

hipError_t launch_tiff(int n, ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, const int32_t* lengths,
                       uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s, uint64_t rm, uint64_t hint) {
  if (!route_on(rm, kRtTiff) || n <= 0) return hipSuccess;
  const unsigned g = route_grid(hint, kRtTiff, n);
  hipLaunchKernelGGL(k_tiff_copy, dim3(g, kTiffStripY), dim3(64), 0, s, descs, blob, offsets, lengths, scratch, routes, cap);
  hipLaunchKernelGGL(k_tiff_lzw, dim3(g, kTiffStripY), dim3(64), 0, s, descs, blob, offsets, lengths, scratch, routes, cap);
  hipLaunchKernelGGL(k_tiff_inflate, dim3(g, kTiffStripY), dim3(64), 0, s, descs, blob, offsets, lengths, scratch, routes, cap);
  hipLaunchKernelGGL(k_tiff_rgb, dim3(g, kTiffRgbSlices), dim3(kTiffRgbThreads), 0, s, descs, blob, offsets, scratch, routes, cap);
  return hipGetLastError();
}

}  // namespace sdsj

extern "C" int sdsj_tiff_probe(const uint8_t* tiff, size_t n, sdsj_tiff_info* out) {
  if (!tiff || !out) return SDSJ_EINVAL;
  memset(out, 0, sizeof(*out));
  sdsj::TiffHdr h;
  const sdsj::GlobalReader rd{tiff};
  const int st = sdsj::tiff_parse(rd, (int64_t)n, &h);
  out->width = h.width;
  out->height = h.height;
  out->samples = h.spp;
  out->photometric = h.photo;
  out->codec = h.codec;
  out->predictor = h.predictor;
  out->rows_per_strip = h.rps;
  out->strips = h.nstrips;
  out->supported = st == SDSJ_OK;
  return st;
}
