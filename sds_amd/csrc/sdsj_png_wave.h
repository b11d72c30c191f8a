// sdsj_png_wave.h -- the wavefront-level pieces the PNG kernels of sdsj_png.hip (base subset),
// sdsj_png_ext.hip (SDSJ_FORMAT_PNG_EXT) and sdsj_png_meta.hip (SDSJ_FORMAT_PNG_META) share: readers, the
// inflate sink, Adler-32.  Device code only; every correctness decision is in sdsj_png.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// Bit depth and interlace method of a PNG descriptor (png_fill_desc keeps them in png_depth_lace).
struct PngIhdr {
  int depth, interlace;
};
__device__ __forceinline__ PngIhdr png_ihdr(const ImgDesc* d) { return PngIhdr{d->png_depth_lace & 255, (d->png_depth_lace >> 8) & 255}; }
__device__ __forceinline__ bool png_plain(const ImgDesc* d) { return d->png_depth_lace == 8; }  // depth 8, not interlaced

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

// A filter type above 4 in the first byte of any row of any pass, lane l looking at rows l, l + 64, ...
// (not inlined: the walk over the passes stays out of the inflate kernel's register budget;
// sdsj_png_inflate_kernel.h says which kernels call it).
__device__ __noinline__ bool wave_filter_bytes_bad(const uint8_t* out, int w, int h, int ctype, PngIhdr ih, int lane) {
  bool bad = false;
  for (int p = 0; p < (ih.interlace ? 7 : 1); p++) {
    PngPass ps;
    if (!png_pass_at(w, h, ctype, ih.depth, ih.interlace, p, &ps)) continue;
    const int64_t pitch = 1 + ps.rowbytes;
    for (int y = lane; y < ps.h; y += 64) bad |= out[ps.off + (int64_t)y * pitch] > 4;
  }
  return bad;
}

}  // namespace

}  // namespace sdsj
