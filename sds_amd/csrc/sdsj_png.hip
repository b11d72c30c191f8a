// sdsj_png.hip -- gfx950 kernels of the opt-in PNG path (SDSJ_FORMAT_PNG) and sdsj_png_probe.
//
//   k_png_inflate   one wavefront per image: zlib / deflate over the IDAT chain into the image's
//                   scanline buffer (scratch, off_png), Adler-32 and the rows' filter bytes checked
//   k_png_unfilter  one wavefront per image: filters 0-4 reversed, RGB rows written to off_rgb (gray
//                   replicated, palette looked up, alpha dropped), which k_hpass / k_vpass then read
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

namespace sdsj {

namespace {

struct GlobalReader {
  const uint8_t* g;
  __device__ __host__ int operator()(int64_t i) const { return g[i]; }
};

// The inflate kernel's input: a window of kWin bytes of the sample staged in LDS by all lanes (coalesced
// byte loads, none at or beyond the sample's length), so the bit reader's byte reads cost an LDS access
// instead of a dependent global load each.  Every lane asks for the same byte at the same time.
constexpr int kWin = 1024;
struct WindowReader {
  const uint8_t* g;
  int64_t n;
  uint8_t* win;
  int lane;
  mutable int64_t w0;
  __device__ __forceinline__ int operator()(int64_t i) const {
    if (i < w0 || i >= w0 + kWin) {
      __syncthreads();  // (one wave per block: earlier reads of the window are done)
      w0 = (i & ~(int64_t)63) - 64;  // (a refill that looks a few bytes ahead does not lose the bytes before)
#pragma unroll
      for (int k = 0; k < kWin / 64; k++) {
        const int64_t j = w0 + k * 64 + lane;
        if (j >= 0 && j < n) win[k * 64 + lane] = g[j];
      }
      __syncthreads();
    }
    return win[i - w0];
  }
};

// Stores of this wave must have completed before its later loads of the same bytes (match sources,
// the Adler pass, the previous band's last row): a workgroup-scope release / acquire pair, which on
// this target is a wait for the wave's outstanding vector memory operations; the wave reads back
// through its own CU's L1, which its stores write through.
__device__ __forceinline__ void wave_store_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The inflate sink of a wavefront.  Every lane runs the (wave-uniform) decode and holds the same
// state; literals are batched -- lane k keeps the k-th pending byte -- and leave as one store of up
// to 64 consecutive bytes; a match is copied by all lanes, 64 bytes per step.  png_inflate has
// validated every position before the sink sees it.
struct WaveSink {
  uint8_t* out;
  int64_t pos;  // bytes stored
  int nl;       // pending literals
  uint32_t mine;
  int lane;
  __device__ __forceinline__ void flush() {
    if (lane < nl) out[pos + lane] = (uint8_t)mine;
    pos += nl;
    nl = 0;
  }
  __device__ __forceinline__ void lit(int b) {
    if (lane == nl) mine = (uint32_t)b;
    if (++nl == 64) flush();
  }
  __device__ __forceinline__ void match(int dist, int len) {
    flush();
    wave_store_fence();
    const uint8_t* src = out + pos - dist;
    if (dist >= len) {
      for (int i = lane; i < len; i += 64) out[pos + i] = src[i];
    } else {  // overlapped: the source repeats with period dist, all of it stored before this match
      for (int i = lane; i < len; i += 64) out[pos + i] = src[i % dist];
    }
    pos += len;
  }
};

// Adler-32 of p[0, n) by one wave: lane l sums its contiguous segment (s1 and s2 from zero), the
// segments are then chained in lane order.
__device__ uint32_t wave_adler(const uint8_t* p, int64_t n, int lane) {
  const int64_t seg = align_up((n + 63) / 64, 4);
  int64_t i0 = (int64_t)lane * seg, i1 = i0 + seg;
  i0 = i0 < n ? i0 : n;
  i1 = i1 < n ? i1 : n;
  uint64_t a = 0, s2 = 0;
  int64_t i = i0;
  for (; i + 4 <= i1; i += 4) {  // (p is 256-byte aligned and seg a multiple of 4)
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p + i);
    a += v & 255;
    s2 += a;
    a += (v >> 8) & 255;
    s2 += a;
    a += (v >> 16) & 255;
    s2 += a;
    a += v >> 24;
    s2 += a;
  }
  for (; i < i1; i++) {
    a += p[i];
    s2 += a;
  }
  const uint32_t al = (uint32_t)(a % kAdlerMod), bl = (uint32_t)(s2 % kAdlerMod), ll = (uint32_t)((i1 - i0) % kAdlerMod);
  uint32_t S1 = 1, S2 = 0;
  for (int l = 0; l < 64; l++) {
    const uint32_t xa = __shfl(al, l), xb = __shfl(bl, l), xl = __shfl(ll, l);
    S2 = (uint32_t)((S2 + (uint64_t)S1 * xl + xb) % kAdlerMod);
    S1 = (S1 + xa) % kAdlerMod;
  }
  return (S2 << 16) | S1;
}

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) k_png_inflate(ImgDesc* __restrict__ descs, const uint8_t* __restrict__ blob,
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
    sink.flush();
    wave_store_fence();
    if (st == SDSJ_OK) {
      if (wave_adler(out, expect, lane) != want) st = SDSJ_CORRUPT;
      // a filter type above 4 is an error in ZipDecode.c
      const int64_t pitch = 1 + (int64_t)d->width * d->png_bpp;
      bool bad = false;
      for (int y = lane; y < d->height; y += 64) bad |= out[(int64_t)y * pitch] > 4;
      if (__ballot(bad)) st = SDSJ_CORRUPT;
    }
    __syncthreads();  // T is rebuilt by the next image
    if (st != SDSJ_OK && lane == 0) d->status = st;
  }
}

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
    if (d->status != SDSJ_OK || !d->png || d->geo == kGeoZeros) continue;
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
                      hipEvent_t between) {
  if (!route_on(rm, kRtPng)) {
    if (between) (void)hipEventRecord(between, s);
    return hipSuccess;
  }
  const unsigned g = route_grid(hint, kRtPng, n);
  hipLaunchKernelGGL(k_png_inflate, dim3(g), dim3(64), 0, s, descs, blob, offsets, lengths, scratch, routes, cap);
  if (between) (void)hipEventRecord(between, s);
  hipLaunchKernelGGL(k_png_unfilter, dim3(g), dim3(64), 0, s, descs, blob, offsets, scratch, routes, cap);
  return hipGetLastError();
}

}  // namespace sdsj

extern "C" int sdsj_png_probe(const uint8_t* png, size_t n, sdsj_png_info* out) {
  if (!png || !out) return SDSJ_EINVAL;
  memset(out, 0, sizeof(*out));
  sdsj::PngHdr h;
  const sdsj::GlobalReader rd{png};
  const int st = sdsj::png_parse(rd, (int64_t)n, &h);
  out->width = h.width;
  out->height = h.height;
  out->bit_depth = h.bit_depth;
  out->color_type = h.ctype;
  out->interlace = h.interlace;
  out->supported = st == SDSJ_OK;
  return st;
}
