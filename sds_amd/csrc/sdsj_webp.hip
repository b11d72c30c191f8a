// sdsj_webp.hip -- gfx950 kernels of the opt-in lossless WebP path (SDSJ_FORMAT_WEBP) and sdsj_webp_probe.
//
//   k_webp_decode   one wavefront per image: transforms' data, prefix codes and the LZ77 / colour-cache
//                   coded ARGB image into the sample's scratch (off_png, laid out by webp_layout)
//   k_webp_inverse  one wavefront per image: the inverse transforms, in place, in reverse order of reading,
//                   over rows [0, min(height, src_y1)); the predictor as a skewed wavefront over bands of 64 rows
//   k_webp_rgb      RGB rows [src_y0, src_y1) x [src_x0, src_x0 + src_w) written to off_rgb, alpha dropped,
//                   which k_hpass / k_vpass then read
// launch_webp is called by the engine only when its mask has the bit.
//
// Reference behaviour: PIL.Image.open(...).convert("RGB").  Every correctness and bounds decision is taken by
// the shared functions of sdsj_webp.h (the same ones the sanitizer driver runs serially on the host); the
// kernels below only move pixels with 64 lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sdsj_common.h"
#include "sdsj_kernels.h"
#include "sdsj_png_wave.h"
#include "sdsj_webp.h"

namespace sdsj {

namespace {

constexpr int kWebpCache = 1 << kWebpMaxCacheBits;

// The 32-bit sink of a wavefront, next to WaveSink.  The decode is wave-uniform: every lane holds the same
// state.  Literals are batched -- lane k keeps the k-th pending pixel -- and leave as one store of up to 64
// words; a copy is made by all lanes, 64 pixels per step.  The colour cache sits in LDS.  A literal enters
// it at once (all lanes store the same word).  The 64 pixels of a copy step enter it together, and where two
// of them hash to one slot the later pixel must win, as it does serially: every lane claims its slot with
// the maximum of lane + 1, and only the lane whose claim stands stores.
struct WaveSink32 {
  uint32_t* out;
  int64_t pos;
  int nl;
  uint32_t mine;
  int lane;
  uint32_t* cache;  // kWebpCache words
  uint32_t* claim;  // kWebpCache words, zero between copies
  int cache_bits;
  __device__ __forceinline__ uint32_t slot(uint32_t v) const { return (0x1E35A7BDu * v) >> (32 - cache_bits); }
  __device__ __forceinline__ void begin(uint32_t* dst, int bits) {
    out = dst;
    pos = 0;
    nl = 0;
    cache_bits = bits;
    if (bits)
      for (int i = lane; i < (1 << bits); i += 64) cache[i] = 0u;
    __syncthreads();
  }
  __device__ __forceinline__ void flush() {
    if (lane < nl) out[pos + lane] = mine;
    pos += nl;
    nl = 0;
  }
  __device__ __forceinline__ void lit(uint32_t v) {
    if (cache_bits) cache[slot(v)] = v;
    if (lane == nl) mine = v;
    if (++nl == 64) flush();
  }
  __device__ __forceinline__ void cached(int key) { lit(cache[key]); }
  __device__ __forceinline__ void match(int dist, int len) {
    flush();
    wave_store_fence();
    const uint32_t* src = out + pos - dist;
    for (int base = 0; base < len; base += 64) {
      const int i = base + lane;
      const bool on = i < len;
      uint32_t v = 0;
      if (on) {  // (overlapped: the source repeats with period dist, all of it stored before this copy)
        v = src[dist >= len ? i : i % dist];
        out[pos + i] = v;
      }
      if (cache_bits) {
        const uint32_t k = slot(v);
        if (on) atomicMax(&claim[k], (uint32_t)lane + 1u);
        __syncthreads();
        if (on && claim[k] == (uint32_t)lane + 1u) cache[k] = v;
        __syncthreads();
        if (on) claim[k] = 0u;
        __syncthreads();
      }
    }
    pos += len;
  }
  __device__ __forceinline__ void finish() {
    flush();
    wave_store_fence();
  }
  // a group's tables from the scratch, where this wave built them, into LDS
  __device__ __forceinline__ void load_codes(WebpCode* dst, const WebpCode* src) {
    wave_store_fence();
    __syncthreads();  // (reads of the previous group's tables are done)
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (int i = lane; i < (int)(5 * sizeof(WebpCode) / 4); i += 64) d[i] = s[i];
    __syncthreads();
  }
  __device__ __forceinline__ int max_group(const uint32_t* p, int64_t n) const {
    uint32_t m = 0;
    for (int64_t i = lane; i < n; i += 64) {
      const uint32_t g = (p[i] >> 8) & 0xFFFFu;
      m = g > m ? g : m;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t x = (uint32_t)__shfl_xor((int)m, o);
      m = x > m ? x : m;
    }
    return (int)m;
  }
};

// LDS per wave: the colour cache and its claims (8 KiB each), the lengths being read and the current group's
// five lookup tables (WebpTmp, 5.6 KiB) and the 1 KiB window of the input: 23 KiB, so six waves share a CU's
// 160 KiB.  The groups' tables are built in the sample's scratch (9 KiB a group); the group in use has its
// lookup tables copied to LDS, so that a symbol costs LDS reads, and only a code longer than 8 bits reads its
// symbol from the scratch.
__global__ void __launch_bounds__(64) k_webp_decode(ImgDesc* __restrict__ descs, const uint8_t* __restrict__ blob,
                                                    const int64_t* __restrict__ offsets, const int32_t* __restrict__ lengths,
                                                    uint8_t* scratch, const int32_t* __restrict__ routes, int cap) {
  __shared__ uint32_t cache[kWebpCache];
  __shared__ uint32_t claim[kWebpCache];
  __shared__ WebpTmp T;
  __shared__ uint8_t win[kWin];
  const int32_t* rl = route_list(routes, cap, kRtWebp);
  const int lane = threadIdx.x;
  for (int i = lane; i < kWebpCache; i += 64) claim[i] = 0u;
  __syncthreads();
  for (int li = blockIdx.x; li < routes[kRtWebp]; li += gridDim.x) {
    const int img = rl[li];
    ImgDesc* d = &descs[img];
    if (d->status != SDSJ_OK || d->png != kWebpSample) continue;
    const WebpView v = webp_view(*d);
    const int64_t n = (int64_t)lengths[img];
    int st = SDSJ_CORRUPT;
    // (webp_parse: the payload lies inside the sample; plan_sample: the scratch is webp_layout's)
    if (d->width > 0 && d->height > 0 && v.data_pos >= 0 && v.data_end <= n && v.data_pos <= v.data_end &&
        d->png_raw == webp_layout(d->width, d->height).total) {
      const WindowReader rd{blob + offsets[img], n, win, lane, -(int64_t)4 * kWin};
      WaveSink32 sink{nullptr, 0, 0, 0u, lane, cache, claim, 0};
      st = webp_decode(rd, v, d->width, d->height, scratch + d->off_png, &T, sink);
    }
    __syncthreads();  // the LDS is the next image's
    if (st != SDSJ_OK && lane == 0) d->status = st;
  }
}

// The rows the resample reads end at src_y1: rows below it are never inverse-transformed (every transform's
// row y needs rows at or above y only).
__global__ void __launch_bounds__(64) k_webp_inverse(const ImgDesc* __restrict__ descs, uint8_t* scratch,
                                                     const int32_t* __restrict__ routes, int cap) {
  const int32_t* rl = route_list(routes, cap, kRtWebp);
  const int lane = threadIdx.x;
  for (int li = blockIdx.x; li < routes[kRtWebp]; li += gridDim.x) {
    const int img = rl[li];
    const ImgDesc* d = &descs[img];
    if (d->status != SDSJ_OK || d->png != kWebpSample || d->geo == kGeoZeros) continue;
    const int width = d->width, height = d->height;
    const int rows = d->src_y1 < height ? d->src_y1 : height;
    if (rows <= 0) continue;
    uint8_t* mem = scratch + d->off_png;
    const WebpLayout L = webp_layout(width, height);
    const WebpState* S = reinterpret_cast<const WebpState*>(mem + L.state);
    uint32_t* a = reinterpret_cast<uint32_t*>(mem + L.argb);
    const uint32_t* ctab = reinterpret_cast<const uint32_t*>(mem + L.ctab);
    for (int ti = S->ntrans - 1; ti >= 0; ti--) {
      const int xs = S->xsize[ti], bits = S->bits[ti], type = S->type[ti];
      const int64_t total = (int64_t)xs * rows;
      const int sw = (xs + (1 << bits) - 1) >> bits;
      if (type == 2) {
        for (int64_t p = lane; p < total; p += 64) a[p] = webp_add_green(a[p]);
      } else if (type == 1) {
        const uint32_t* sub = reinterpret_cast<const uint32_t*>(mem + L.sub[2]);
        for (int64_t p = lane; p < total; p += 64) {
          const int y = (int)(p / xs), x = (int)(p - (int64_t)y * xs);
          a[p] = webp_cross(sub[(int64_t)(y >> bits) * sw + (x >> bits)], a[p]);
        }
      } else if (type == 3) {
        // in place, 64 pixels per step from the last to the first: a step's packed words lie at or below its
        // own pixels, so a later step (lower pixels) never reads what an earlier one stored.  Within a step a
        // lane's pixel can be another lane's packed word: every lane holds its pixel in a register before the
        // barrier, and stores after it.
        for (int64_t base = (total - 1) & ~(int64_t)63; base >= 0; base -= 64) {
          const int64_t p = base + lane;
          uint32_t px = 0;
          if (p < total) {
            const int y = (int)(p / xs), x = (int)(p - (int64_t)y * xs);
            px = webp_indexed(ctab, a[(int64_t)y * sw + (x >> bits)], x, bits);
          }
          __syncthreads();
          if (p < total) a[p] = px;
          __syncthreads();
        }
      } else {
        // Predictor: lane l takes row y0 + l of a band of 64 rows and lags two pixels behind the lane above,
        // so that when it stands at x the lane above has finished x + 1 (TR).  L is the lane's own last
        // result; every step each lane takes the result the lane above produced one step earlier (one
        // ds_bpermute), which is its TR now, its T one step later and its TL two steps later.  Lane 0 reads
        // the row above the band from memory, 64 pixels at a time, after the fence that ended that band.
        const uint32_t* sub = reinterpret_cast<const uint32_t*>(mem + L.sub[1]);
        for (int y0 = 0; y0 < rows; y0 += 64) {
          const int nrows = rows - y0 < 64 ? rows - y0 : 64;
          const int steps = xs + 2 * (nrows - 1);
          const int y = y0 + lane;
          const bool row_on = lane < nrows;
          const uint32_t* above = a + (int64_t)(y0 - 1) * xs;  // (read only when y0 > 0)
          uint32_t left = 0, first = 0, tl = 0, tt = 0, tr = y0 > 0 ? above[0] : 0u, res = 0, top = 0;
          for (int t = 0; t < steps; t++) {
            if ((t & 63) == 0 && y0 > 0) {
              const int xx = t + 1 + lane;
              top = xx < xs ? above[xx] : 0u;
            }
            const uint32_t up = (uint32_t)__shfl_up((int)res, 1);
            const uint32_t topv = (uint32_t)__shfl((int)top, t & 63);
            tl = tt;
            tt = tr;
            tr = lane == 0 ? topv : up;
            const int x = t - 2 * lane;
            if (row_on && x >= 0 && x < xs) {
              const int64_t p = (int64_t)y * xs + x;
              const int mode = webp_border_mode((int)((sub[(int64_t)(y >> bits) * sw + (x >> bits)] >> 8) & 15u), x, y);
              // (past the row's end TR is the memory position after it: the first pixel of this row)
              res = webp_add(a[p], webp_predict(mode, left, tt, tl, x == xs - 1 ? first : tr));
              a[p] = res;
              left = res;
              if (x == 0) first = res;
            }
          }
          wave_store_fence();
        }
      }
      wave_store_fence();
    }
  }
}

// One workgroup per (image, row slice); a thread per pixel of the rows and columns the resample needs.
constexpr int kWebpRgbThreads = 256, kWebpRgbSlices = 8;
__global__ void __launch_bounds__(kWebpRgbThreads) k_webp_rgb(const ImgDesc* __restrict__ descs, uint8_t* scratch,
                                                              const int32_t* __restrict__ routes, int cap) {
  const int32_t* rl = route_list(routes, cap, kRtWebp);
  for (int li = blockIdx.x; li < routes[kRtWebp]; li += gridDim.x) {
    const int img = rl[li];
    const ImgDesc* d = &descs[img];
    if (d->status != SDSJ_OK || d->png != kWebpSample || d->geo == kGeoZeros) continue;
    const int y0 = d->src_y0 < 0 ? 0 : d->src_y0, y1 = d->src_y1 < d->height ? d->src_y1 : d->height;
    const int x0 = d->src_x0, sw = d->src_w;
    if (x0 < 0 || sw <= 0 || x0 + sw > d->width || y1 <= y0) continue;
    const uint32_t* a = reinterpret_cast<const uint32_t*>(scratch + d->off_png + webp_layout(d->width, d->height).argb);
    uint8_t* rgb = scratch + d->off_rgb;
    const int rows = y1 - y0, per = (rows + kWebpRgbSlices - 1) / kWebpRgbSlices;
    const int r0 = blockIdx.y * per, r1 = r0 + per < rows ? r0 + per : rows;
    const int64_t p0 = (int64_t)r0 * sw, p1 = (int64_t)r1 * sw;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += kWebpRgbThreads) {
      const int ry = (int)(p / sw), rx = (int)(p - (int64_t)ry * sw);
      const uint32_t c = a[(int64_t)(y0 + ry) * d->width + x0 + rx];
      uint8_t* o = rgb + ((int64_t)(y0 + ry - d->src_y0) * sw + rx) * 3;
      o[0] = (uint8_t)(c >> 16);
      o[1] = (uint8_t)(c >> 8);
      o[2] = (uint8_t)c;
    }
  }
}

}  // namespace

hipError_t launch_webp(int n, ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, const int32_t* lengths,
                       uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s, uint64_t rm, uint64_t hint) {
  if (!route_on(rm, kRtWebp) || n <= 0) return hipSuccess;
  const unsigned g = route_grid(hint, kRtWebp, n);
  hipLaunchKernelGGL(k_webp_decode, dim3(g), dim3(64), 0, s, descs, blob, offsets, lengths, scratch, routes, cap);
  hipLaunchKernelGGL(k_webp_inverse, dim3(g), dim3(64), 0, s, descs, scratch, routes, cap);
  hipLaunchKernelGGL(k_webp_rgb, dim3(g, kWebpRgbSlices), dim3(kWebpRgbThreads), 0, s, descs, scratch, routes, cap);
  return hipGetLastError();
}

}  // namespace sdsj

extern "C" int sdsj_webp_probe(const uint8_t* webp, size_t n, sdsj_webp_info* out) {
  if (!webp || !out) return SDSJ_EINVAL;
  memset(out, 0, sizeof(*out));
  sdsj::WebpHdr h;
  const sdsj::GlobalReader rd{webp};
  const int st = sdsj::webp_parse(rd, (int64_t)n, &h);
  out->width = h.width;
  out->height = h.height;
  out->has_alpha = h.has_alpha;
  out->lossless = h.lossless;
  out->extended = h.extended;
  out->supported = st == SDSJ_OK;
  return st;
}
