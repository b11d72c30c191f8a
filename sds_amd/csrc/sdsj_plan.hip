// sdsj_plan.hip -- gfx950 (MI355X) kernels around the planner (sdsj_plan.h): header parse and planning on the
// device, status and zero fill at the end of a batch, and host-side planning.
//
// Stage map (reference behaviour each kernel reproduces, see DESIGN.md for the layout/rooflines):
//   k_parse    markers, tables, geometry          jdmarker.c / jdhuff.c tables / functional.py:118-140
//   k_plan     per-batch scratch offsets          (no reference counterpart)
//   k_finish   statuses, per-process counters     (no reference counterpart)
//   k_zerofill zeros of failed samples, empty crops  presets.py:160-162
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdsj_common.h"
#include "sdsj_kernels.h"
#include "sdsj_plan.h"

#pragma clang fp contract(off)

namespace sdsj {

// ------------------------------------------------------------------------------------------
// k_parse: one wave per image.  The first kHdrStage bytes are staged into LDS (coalesced); lane 0
// walks the markers; all lanes build the derived Huffman tables.
// ------------------------------------------------------------------------------------------
constexpr int kHdrStage = 4096;

struct DevReader {
  const uint8_t* lds;
  int64_t nlds;
  const uint8_t* g;
  __device__ int operator()(int64_t i) const { return i < nlds ? lds[i] : g[i]; }
};

// Device sink of the shared parser: lane 0 records the DHT/DQT copies (the last definition of a
// table wins, as with sequential copying); every lane then performs them.
struct ParseJob {
  int32_t kind;  // 0 DHT values, 1 DQT entries (pq = 0), 2 DQT entries (pq = 1)
  int32_t cnt;
  int64_t src;
  void* dst;
};
constexpr int kMaxJobs = 16;

struct DevSink {
  ParseJob* jobs;
  int* njobs;
  const DevReader& rd;
  __device__ void add(int kind, void* dst, int64_t src, int cnt) const {
    for (int q = 0; q < *njobs; q++)
      if (jobs[q].dst == dst) {
        jobs[q] = ParseJob{kind, cnt, src, dst};
        return;
      }
    if (*njobs < kMaxJobs) {
      jobs[(*njobs)++] = ParseJob{kind, cnt, src, dst};
      return;
    }
    // (more distinct tables than kMaxJobs cannot happen: 8 Huffman + 4 quantisation tables)
  }
  __device__ void dht(HuffSpec* h, int64_t src, int cnt) const { add(0, h->vals, src, cnt); }
  __device__ void dqt(uint16_t* qt, int pq, int64_t src) const { add(pq ? 2 : 1, qt, src, 64); }
};

__global__ void __launch_bounds__(64) k_parse(int n, const uint8_t* __restrict__ blob, int64_t blob_bytes,
                                              const int64_t* __restrict__ offsets, const int32_t* __restrict__ lengths,
                                              sdsj_op op, int warm_bits, int small, ImgDesc* __restrict__ descs,
                                              ImgTables* __restrict__ tables, int formats) {
  const int img = blockIdx.x;
  if (img >= n) return;
  const int lane = threadIdx.x;
  {  // the sample's range must lie inside the blob (nothing below reads outside it); otherwise EINVAL
    const int64_t o = offsets[img], l = lengths[img];
    if (o < 0 || l < 0 || o > blob_bytes || l > blob_bytes - o) {
      if (lane == 0) descs[img].status = SDSJ_EINVAL;
      return;
    }
  }
  __shared__ alignas(16) uint8_t hdr[kHdrStage];
  __shared__ ImgDesc sd;
  __shared__ ImgTables st;
  __shared__ ParseJob jobs[kMaxJobs];
  __shared__ int njobs, s_status;

  const uint8_t* g = blob + offsets[img];
  const int64_t len = lengths[img];
  const int64_t nstage = len < kHdrStage ? len : kHdrStage;
  for (int64_t i = lane; i < nstage; i += 64) hdr[i] = g[i];
  if (lane == 0) njobs = 0;
  __syncthreads();
  DevReader rd{hdr, nstage, g};
  if (lane == 0) {
    DevSink sink{jobs, &njobs, rd};
    const int status = plan_sample(rd, len, op, small != 0, formats, &sd, &st, sink);
    if (warm_bits >= 0) sd.warm_bits = warm_bits;  // override (experiments)
    else if (n < kWarmSmallLane && !sd.lat) sd.warm_bits = warm_for(sd.sub_bits, kWarmBitsSmall);  // small lane
    sd.status = status;
    for (int k = 0; k < 4; k++) sd.t_rs[k] = 0;
    s_status = status;
  }
  __syncthreads();
  // the recorded table copies, all lanes (values beyond a DHT's count are zero, jdmarker.c get_dht)
  const int nj = njobs;
  for (int q = 0; q < nj; q++) {
    const ParseJob jb = jobs[q];
    if (jb.kind == 0) {
      uint8_t* v = static_cast<uint8_t*>(jb.dst);
      for (int i = lane; i < 256; i += 64) v[i] = i < jb.cnt ? (uint8_t)rd(jb.src + i) : 0;
    } else {
      uint16_t* qt = static_cast<uint16_t*>(jb.dst);
      const int i = lane;
      qt[natural_order(i)] = (uint16_t)(jb.kind == 2 ? ((rd(jb.src + 2 * i) << 8) | rd(jb.src + 2 * i + 1)) : rd(jb.src + i));
    }
  }
  __syncthreads();
  // validation of the tables the scan uses (jdhuff.c jpeg_make_d_derived_tbl), one lane per table
  if (s_status == SDSJ_OK && !sd.progressive && lane < 2 * sd.ncomp) {
    const int c = lane >> 1;
    const bool dc = (lane & 1) == 0;
    const HuffSpec& h = dc ? st.dc_spec[sd.comp[c].td] : st.ac_spec[sd.comp[c].ta];
    if (!huff_table_ok(h, dc)) sd.status = SDSJ_CORRUPT;
  }
  __syncthreads();
  // write back
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&st);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&tables[img]);
    for (int i = lane; i < (int)(sizeof(ImgTables) / 4); i += 64) dst[i] = src[i];
    const uint32_t* s2 = reinterpret_cast<const uint32_t*>(&sd);
    uint32_t* d2 = reinterpret_cast<uint32_t*>(&descs[img]);
    for (int i = lane; i < (int)(sizeof(ImgDesc) / 4); i += 64) d2[i] = s2[i];
  }
}

// ------------------------------------------------------------------------------------------
// k_plan: one workgroup; exclusive scan of per-image scratch needs -> absolute offsets.
// ------------------------------------------------------------------------------------------
// k_plan, in two kernels.  k_plan_scan (one workgroup): exclusive scan of the images' scratch needs
// from the previous lane's total (each image's plan_base, the lane's total), route counters zeroed.
// k_plan_apply (one thread per image): capacity check, the image's scratch offsets, its route-list
// entries -- counted per workgroup in LDS, one global atomic per route and workgroup (the lists'
// order is the workgroups' arrival order; every image still lands in exactly its lists).
__global__ void __launch_bounds__(1024) k_plan_scan(int n, ImgDesc* __restrict__ descs, const int64_t* __restrict__ base,
                                                    int64_t* __restrict__ total_out, int32_t* __restrict__ routes) {
  __shared__ int64_t part[1024];
  __shared__ int64_t carry;
  const int t = threadIdx.x;
  if (t == 0) carry = base ? *base : 0;  // a second lane allocates after the first
  if (t < kRouteSlots) routes[t] = 0;    // route counts, then work counters
  __syncthreads();
  for (int b0 = 0; b0 < n; b0 += 1024) {
    const int i = b0 + t;
    int64_t need = 0;
    if (i < n && descs[i].status == SDSJ_OK) need = descs[i].need;
    part[t] = need;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int64_t v = t >= off ? part[t - off] : 0;
      __syncthreads();
      part[t] += v;
      __syncthreads();
    }
    if (i < n) descs[i].plan_base = carry + part[t] - need;
    __syncthreads();
    if (t == 1023) carry += part[1023];
    __syncthreads();
  }
  if (t == 0) *total_out = carry;
}

constexpr int kPlanThreads = 256;
__global__ void __launch_bounds__(kPlanThreads) k_plan_apply(int n, ImgDesc* __restrict__ descs, int64_t capacity,
                                                             int32_t* __restrict__ routes, int cap) {
  __shared__ int lcnt[kNumRoutes], gbase[kNumRoutes];
  const int t = threadIdx.x, i = blockIdx.x * kPlanThreads + t;
  if (t < kNumRoutes) lcnt[t] = 0;
  __syncthreads();
  int ru = -1, re = -1, rr = -1, iu = 0, ie = 0, ir = 0, ig = 0, ng = 0;
  if (i < n && descs[i].status == SDSJ_OK) {
    ImgDesc& d = descs[i];
    const int64_t start = d.plan_base;
    if (start + d.need > capacity) {
      d.status = SDSJ_ECAPACITY;
    } else {
      d.off_ustream += start;
      d.off_seg += start;
      d.off_tiles += start;
      d.off_sub += start;
      d.off_rec += start;
      d.off_ptab += start;
      d.off_coef += start;
      d.off_planes += start;
      d.off_rgb += start;
      d.off_tmp += start;
      d.off_kh += start;
      d.off_kv += start;
      d.off_png += start;
      // routes (image_routes): unstuffing -- one workgroup per small image, tile-parallel passes for
      // the rest --, entropy variant, resample variant
      image_routes(d, &ru, &re, &rr);
      if (ru >= 0) iu = atomicAdd(&lcnt[ru], 1);
      ie = atomicAdd(&lcnt[re], 1);
      if (re == kRtEnt11M) {
        ng = d.ent_groups;
        ig = atomicAdd(&lcnt[kRtEnt11G], ng);
      }
      if (rr >= 0) ir = atomicAdd(&lcnt[rr], 1);
    }
  }
  __syncthreads();
  if (t < kNumRoutes) gbase[t] = lcnt[t] ? atomicAdd(&routes[t], lcnt[t]) : 0;
  __syncthreads();
  if (ru >= 0) routes[kRouteSlots + ru * cap + gbase[ru] + iu] = i;
  if (re >= 0) routes[kRouteSlots + re * cap + gbase[re] + ie] = i;
  if (ng) {
    int32_t* gt = group_tasks(routes, cap);
    for (int q = 0; q < ng; q++) gt[gbase[kRtEnt11G] + ig + q] = (i << kGroupShift) | q;
  }
  if (rr >= 0) routes[kRouteSlots + rr * cap + gbase[rr] + ir] = i;
}

// k_finish: publishes every sample's status and accumulates the engine's per-process counters
// (SDSJ_CTR_*): one thread per sample, counters summed in LDS, one 64-bit atomic per counter and
// workgroup (lengths == null: the frames path).  k_zerofill then writes the zeros of failed samples and empty crops
// (presets.py:160-162 normalise maps them to -1.0 through the LUT, as zeros would).
__global__ void __launch_bounds__(256) k_finish(int n, const ImgDesc* __restrict__ descs, sdsj_op op,
                                                int32_t* __restrict__ status, const int32_t* __restrict__ lengths,
                                                unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long acc[SDSJ_NUM_COUNTERS];
  const int t = threadIdx.x, img = blockIdx.x * 256 + t;
  if (t < SDSJ_NUM_COUNTERS) acc[t] = 0;
  __syncthreads();
  const int64_t total = (int64_t)op.out_h * op.out_w * 3;
  if (img < n) {
    const ImgDesc* d = &descs[img];
    const int st = d->status;  // (k_parse: EINVAL for a sample outside the blob / a negative length)
    status[img] = st;
    if (counters) {
      const int k = st == SDSJ_OK ? SDSJ_CTR_OK
                    : st == SDSJ_UNSUPPORTED ? SDSJ_CTR_UNSUPPORTED
                    : st == SDSJ_CORRUPT ? SDSJ_CTR_CORRUPT
                    : st == SDSJ_ECAPACITY ? SDSJ_CTR_CAPACITY : SDSJ_CTR_OTHER;
      atomicAdd(&acc[lengths ? SDSJ_CTR_IMAGES : SDSJ_CTR_FRAMES], 1ull);
      atomicAdd(&acc[k], 1ull);
      if (lengths && lengths[img] > 0) atomicAdd(&acc[SDSJ_CTR_BYTES_IN], (unsigned long long)lengths[img]);
      atomicAdd(&acc[SDSJ_CTR_BYTES_OUT], (unsigned long long)(total * (op.out_dtype == SDSJ_DTYPE_F32 ? 4 : 1)));
      if (lengths && st == SDSJ_OK && d->progressive == 1) atomicAdd(&acc[SDSJ_CTR_PROGRESSIVE], 1ull);
      if (lengths && st == SDSJ_OK && d->png == 1) atomicAdd(&acc[SDSJ_CTR_PNG], 1ull);  // (2: a GIF sample)
    }
  }
  __syncthreads();
  if (counters && t < SDSJ_NUM_COUNTERS && acc[t]) atomicAdd(&counters[t], acc[t]);
}

// k_zerofill: zeros of failed samples and empty crops.  Work items = (image, chunk of 1/kZeroChunks of
// its output); a capped grid strides over them.  A workgroup reads the status of its next 256 items at
// once (one per thread) into LDS and then fills the flagged ones, so a batch without failures costs one
// coalesced descriptor pass (item by item, the status reads were a dependent chain: 84 us per 16,384
// images), and a batch of failures is still filled by the whole grid.
constexpr int kZeroChunks = 16;
constexpr int kZeroGrid = 2048;
__global__ void __launch_bounds__(256) k_zerofill(int n, const ImgDesc* __restrict__ descs, sdsj_op op,
                                                  void* __restrict__ out, const float* __restrict__ lut) {
  __shared__ int32_t fill[256];  // the window's flagged items, compacted
  __shared__ int nfill;
  const int t = threadIdx.x;
  const int64_t total = (int64_t)op.out_h * op.out_w * 3, per = (total + kZeroChunks - 1) / kZeroChunks;
  const int64_t items = (int64_t)n * kZeroChunks;
  for (int64_t k0 = 0; blockIdx.x + k0 * gridDim.x < items; k0 += 256) {
    const int64_t w = blockIdx.x + (k0 + t) * gridDim.x;  // this thread's item of the window
    bool f = false;
    if (w < items) {
      const ImgDesc* d = &descs[w / kZeroChunks];
      f = d->status != SDSJ_OK || d->geo == kGeoZeros;
    }
    if (t == 0) nfill = 0;
    __syncthreads();
    if (f) fill[atomicAdd(&nfill, 1)] = t;  // (a window without failures: one barrier, no loop -- the scan
    __syncthreads();                         //  of all 256 flags cost a single-image call ~10 us)
    for (int q = 0; q < nfill; q++) {
      const int k = fill[q];
      const int64_t wk = blockIdx.x + (k0 + k) * gridDim.x;
      const int img = (int)(wk / kZeroChunks), ch = (int)(wk % kZeroChunks);
      const int64_t e0 = ch * per, e1 = e0 + per < total ? e0 + per : total;
      if (op.out_dtype == SDSJ_DTYPE_F32) {
        float* o = reinterpret_cast<float*>(out) + (int64_t)img * total;
        const float z = lut[0];
        for (int64_t i = e0 + t; i < e1; i += blockDim.x) o[i] = z;
      } else {
        uint8_t* o = reinterpret_cast<uint8_t*>(out) + (int64_t)img * total;
        for (int64_t i = e0 + t; i < e1; i += blockDim.x) o[i] = 0;
      }
    }
    __syncthreads();  // fill reused
  }
}

// ------------------------------------------------------------------------------------------
// Host-side launchers (called by the engine; all asynchronous on `stream`).
// ------------------------------------------------------------------------------------------
hipError_t launch_parse(int n, const uint8_t* blob, int64_t blob_bytes, const int64_t* offsets, const int32_t* lengths,
                        const sdsj_op& op, int warm_bits, bool small, ImgDesc* descs, ImgTables* tables, hipStream_t s,
                        int formats) {
  hipLaunchKernelGGL(k_parse, dim3(n), dim3(64), 0, s, n, blob, blob_bytes, offsets, lengths, op, warm_bits, (int)small,
                     descs, tables, formats);
  return hipGetLastError();
}
hipError_t launch_plan(int n, ImgDesc* descs, int64_t capacity, const int64_t* base, int64_t* total, int32_t* routes,
                       int cap, hipStream_t s) {
  hipLaunchKernelGGL(k_plan_scan, dim3(1), dim3(1024), 0, s, n, descs, base, total, routes);
  if (n > 0)
    hipLaunchKernelGGL(k_plan_apply, dim3((n + kPlanThreads - 1) / kPlanThreads), dim3(kPlanThreads), 0, s, n, descs,
                       capacity, routes, cap);
  return hipGetLastError();
}
hipError_t launch_finish(int n, ImgDesc* descs, const sdsj_op& op, void* out, int32_t* status, const float* lut,
                         const int32_t* lengths, unsigned long long* counters, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_finish, dim3((n + 255) / 256), dim3(256), 0, s, n, descs, op, status, lengths, counters);
  const int zg = n * kZeroChunks < kZeroGrid ? n * kZeroChunks : kZeroGrid;
  hipLaunchKernelGGL(k_zerofill, dim3(zg), dim3(256), 0, s, n, descs, op, out, lut);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Host-side planning (the engine's host paths: scratch needs and route masks before the launch).
// ------------------------------------------------------------------------------------------
int64_t host_plan_frame(ImgDesc* d, int width, int height, const sdsj_op& op) {
  *d = ImgDesc{};
  d->status = SDSJ_OK;
  d->width = width;
  d->height = height;
  d->ncomp = 3;
  return plan_image(d, op, true);
}

// The plan k_parse makes (plan_sample), without k_parse's validation of the Huffman tables: a sample
// whose tables are bad is sized and routed here like a good one and reported by the device.  It stays
// that way: sdsj_plan_need / sdsj_plan_need_formats return these statuses and needs.  A multi-scan
// sequential file that k_scans refuses while it walks the scans -- after k_plan has given it its scratch -- is
// such a sample too: status SDSJ_OK and its need here, the refusal (scans_check) in *later.
int64_t host_plan_need(const uint8_t* jpg, int64_t n, const sdsj_op& op, int* status, uint64_t* routes, bool small,
                       int formats, int* later) {
  ImgDesc d;
  static thread_local ImgTables t;
  MemReader rd{jpg};
  int st = plan_sample(rd, n, op, small, formats, &d, &t, CopySink<MemReader>{rd});
  // (the device runs this check in a kernel of its own between k_parse and k_plan: launch_png_meta)
  if (st == SDSJ_OK && d.png == 1 && (formats & SDSJ_FORMAT_PNG_META)) st = host_png_meta(jpg, n, d.png_idat_pos, formats);
  *status = st;
  if (later) *later = st == SDSJ_OK && !d.png && d.progressive == kScansSequential ? scans_check(rd, n, d) : SDSJ_OK;
  if (routes) {
    *routes = kAllRoutes;
    if (st == SDSJ_OK) {
      int ru, re, rr;
      image_routes(d, &ru, &re, &rr);
      *routes = (ru >= 0 ? 1ull << ru : 0) | (1ull << re) | (rr >= 0 ? 1ull << rr : 0);
    }
  }
  return st == SDSJ_OK ? d.need : 0;
}

}  // namespace sdsj
