// sdsj_engine.hip -- the C-ABI (include/sdsj.h): engine state, scratch management, batch driver.
//
// One engine per process and device (sds transforms are created lazily per DataLoader worker,
// presets.py:1-5).  The engine owns device scratch, per-image descriptor/table arrays, the host
// paths' staging and the 256-entry normalisation LUT, each through an owner of sdsj_buffers.h:
// deleting the engine releases everything.  Every batch is a fixed sequence of kernel launches on
// the caller's stream: no host synchronisation inside the device-resident entry point.
//
// Host paths.  sdsj_decode_resize_batch (one Staging, a chunk of max_batch at a time) and
// sdsj_submit_batch / sdsj_submit_files (one Staging per slot) share one layout and one set of
// helpers: the samples are staged into a pinned region at 16-byte-aligned offsets, followed by their
// offsets, lengths and flip flags (stage_layout); planning runs over that pinned copy; the whole
// region goes to the device with one copy -- on the caller's stream for the synchronous call, on the
// engine's copy stream (joined by an event) for a slot.  An engine takes one host call at a time.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <errno.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "sdsj_buffers.h"
#include "sdsj_common.h"
#include "sdsj_kernels.h"
#include "sdsj_plan.h"
#include "sdsj_stage_pool.h"

using namespace sdsj;

namespace {
constexpr int kStages = 15;
#ifndef SDSJ_MAX_LANES
#define SDSJ_MAX_LANES 4
#endif
constexpr int kMaxLanes = SDSJ_MAX_LANES;
const char* kStageNames[kStages] = {"parse", "plan",  "unstuff", "prog",  "entspec",  "entsync",     "entwrite",    "idct",
                                    "color", "coeffs", "hpass",   "vpass", "resample", "png_inflate", "png_unfilter"};
constexpr int kMarkAfterSpec = 5;  // mark index at the end of the entspec stage
// The PNG kernels run between "prog" and "entspec", but their stages are named last (stage indices are
// part of the interface).  A lane's events are recorded in time order: stage k spans the events
// stage_event(k) and stage_event(k) + 1.
constexpr int kPngEvent = 4;  // events 4, 5: the starts of k_png_inflate and k_png_unfilter
constexpr int stage_event(int k) { return k < 4 ? k : k < 13 ? k + 2 : kPngEvent + (k - 13); }

// One staged batch of the host paths: a pinned region in the packed layout of stage_layout
// (sdsj_buffers.h), its device copy, and the per-sample statuses.
struct Staging {
  PinnedBuf<uint8_t> h;
  DeviceBuf<uint8_t> d;
  PinnedBuf<int32_t> h_status;
  DeviceBuf<int32_t> d_status;
  std::unique_ptr<int32_t[]> pre;  // host-side per-sample status (unreadable files)
  int cap = 0;                     // samples h_status, d_status and pre hold
  StageLayout lay;                 // of the staged batch, n samples
  int n = 0;
  bool pending = false;            // launched and not yet collected
  hipStream_t stream = nullptr;    // the stream of that launch
  Event ev_h2d, ev_done;           // slots only: the copy-stream join and the completion (stage_launch)
  int64_t* offsets() const { return reinterpret_cast<int64_t*>(h.get() + lay.offsets); }
  int32_t* lengths() const { return reinterpret_cast<int32_t*>(h.get() + lay.lengths); }
  uint8_t* flip() const { return h.get() + lay.flip; }
};
}  // namespace

struct sdsj_engine {
  int device = 0;
  int max_batch = 4096;
  bool grow = true;
  int formats = SDSJ_FORMAT_JPEG;  // sdsj_engine_set_formats
  int warm_bits = -1;  // entropy warm-up override (SDSJ_WARM_BITS, experiments); < 0 = plan default
  DeviceBuf<uint8_t> scratch;
  int64_t capacity() const { return (int64_t)scratch.size(); }
  DeviceBuf<ImgDesc> descs;
  DeviceBuf<ImgTables> tables;
  DeviceBuf<int64_t> d_total;
  DeviceBuf<uint8_t> d_etab;    // per-image decode tables built by k_enttab
  DeviceBuf<int32_t> d_routes;  // per-variant image lists built by k_plan (sdsj_common.h Route)
  // lanes 2.. of a chunk (run_chunk): route lists and scratch totals, streams and events
  int lanes = 4;     // SDSJ_LANES (experiments)
  int lane_mid = 2;  // lane k + 1 starts at lane k's mark lane_mid (>= 2: k_plan done; -1: its spec pass)
  DeviceBuf<int64_t> d_totals_x;
  DeviceBuf<int32_t> d_routes_x;
  Stream aux[kMaxLanes - 1];
  Event ev_mid[kMaxLanes - 1], ev_join[kMaxLanes - 1];
  // route hints of the device path (sdsj_kernels.h route_grid), one per op (the resample route -- taps,
  // layout -- follows the output size, filter, dtype and layout): each call copies its lanes' route counts
  // to pinned memory after k_plan; a later call folds a finished copy into the hint of the op it ran
  static constexpr int kHintSlots = 4;
  uint64_t hint_key[kHintSlots] = {};
  uint64_t hint[kHintSlots] = {};
  int hint_n = 0, hint_next = 0;
  PinnedBuf<int32_t> h_rcounts;  // [kMaxLanes][kNumRoutes], then [kMaxLanes]: the lanes' k_enthint miss counts
  Event ev_rc[kMaxLanes];
  bool rc_pending = false;
  int rc_lanes = 0;
  uint64_t rc_key = 0;  // the op of the outstanding readback
  // frames path: host-planned descriptors and route list, staged through pinned memory
  PinnedBuf<ImgDesc> h_fdescs;
  PinnedBuf<int32_t> h_froutes;
  DeviceBuf<float> d_lut;
  DeviceBuf<unsigned long long> d_counters;  // SDSJ_CTR_* (k_finish)
  // entry-point store of the device path (sdsj_common.h HintHdr): hint_rows slots of a key and a record,
  // allocated by the first device-resident call; per-lane work lists; SDSJ_HINT_CTR_*
  int64_t hint_rows = -1;  // < 0: 2 x max_batch
  DeviceBuf<unsigned long long> d_hint_keys;  // [2 x hint_rows]
  DeviceBuf<int32_t> d_hint_ridx;             // [2 x hint_rows], then the record count
  DeviceBuf<uint8_t> d_hint_recs;
  DeviceBuf<int32_t> d_hint_lanes;  // [kMaxLanes][hint_lane_ints(max_batch)]
  DeviceBuf<unsigned long long> d_hint_ctr;
  // host paths: sdsj_decode_resize_batch stages each chunk in `sync_stage`, sdsj_submit_* in slots[slot] with
  // the H2D copy on copy_stream; parallel_for's persistent threads are created on first use
  Staging sync_stage, slots[SDSJ_SLOTS];
  Stream copy_stream;
  std::unique_ptr<StagePool> pool;
  // timing: one event set per chunk launched since the last sdsj_engine_set_timing(e, 1)
  bool timing = false;
  std::vector<std::vector<Event>> ev_sets;
  size_t ev_used = 0;
  std::string err;
};

namespace {

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

int fail(sdsj_engine* e, int code, const std::string& msg) {
  if (e) e->err = msg;
  return code;
}

int hip_fail(sdsj_engine* e, hipError_t st, const char* what) {
  return fail(e, SDSJ_EHIP, std::string(what) + ": " + hipGetErrorString(st));
}

#define SDSJ_HIP(e, call)                                  \
  do {                                                     \
    hipError_t _st = (call);                               \
    if (_st != hipSuccess) return hip_fail((e), _st, #call); \
  } while (0)

// A Buf::reserve failed: the runtime's error for it, as SDSJ_EHIP.
int alloc_fail(sdsj_engine* e, const char* what) { return hip_fail(e, hipGetLastError(), what); }

int ensure_scratch(sdsj_engine* e, int64_t need) {
  if (need <= e->capacity() && e->scratch) return SDSJ_OK;
  int64_t cap = std::max<int64_t>(need, e->capacity() * 3 / 2);
  cap = std::max<int64_t>(cap, 64 << 20);
  if (!e->scratch.reserve((size_t)cap)) return alloc_fail(e, "scratch allocation");
  return SDSJ_OK;
}

// The one place a host-planned batch sizes scratch: grows it to `need` bytes (at least `floor`; after
// the work queued on s, which may still use the old arena), or fails when the capacity was configured.
int scratch_for(sdsj_engine* e, int64_t need, hipStream_t s, const char* too_large, int64_t floor = 0) {
  if (e->scratch && need <= e->capacity()) return SDSJ_OK;
  if (e->scratch && !e->grow) return fail(e, SDSJ_ECAPACITY, too_large);
  SDSJ_HIP(e, hipStreamSynchronize(s));
  return ensure_scratch(e, std::max(need, floor));
}

bool valid_op(const sdsj_op* op) {
  return op && op->out_h > 0 && op->out_w > 0 && op->out_h <= 65535 && op->out_w <= 65535 && op->filter >= 0 &&
         op->filter <= SDSJ_FILTER_NEAREST && (op->out_dtype == SDSJ_DTYPE_U8 || op->out_dtype == SDSJ_DTYPE_F32) &&
         (op->layout == SDSJ_LAYOUT_CHW || op->layout == SDSJ_LAYOUT_HWC);
}

int64_t out_bytes_per_image(const sdsj_op& op) {
  return (int64_t)op.out_h * op.out_w * 3 * (op.out_dtype == SDSJ_DTYPE_F32 ? 4 : 1);
}

// One lane of a chunk: a contiguous range of its images with their own route lists and scratch
// total.  `base`: the scratch bytes the previous lane took (device), or null for the first lane.
struct Lane {
  ImgDesc* descs;
  ImgTables* tables;
  void* etab;
  int32_t* routes;
  int64_t* total;
  const int64_t* base;
};

// Runs the kernel sequence for one lane (n <= max_batch images) of device-resident inputs.
// after_spec (optional) is recorded once the lane's speculative entropy pass is queued.
// hint: routes expected to hold images (full grids); rc_lane >= 0: copy this lane's route counts to the
// engine's pinned readback slot rc_lane after k_plan
int run_lane(sdsj_engine* e, const Lane& ln, int n, bool small, const uint8_t* d_blob, int64_t blob_bytes, const int64_t* d_offsets,
             const int32_t* d_lengths, const sdsj_op& op, const uint8_t* d_flip, void* d_out, int32_t* d_status,
             hipStream_t s, hipEvent_t after_spec, uint64_t rm, uint64_t hint = kAllRoutes, int rc_lane = -1,
             const HintLane* hl = nullptr) {
  std::vector<Event>* evs = nullptr;
  if (e->timing) {
    if (e->ev_used == e->ev_sets.size()) {
      std::vector<Event> set(kStages + 1);  // (in time order: stage_event)
      for (auto& ev : set) SDSJ_HIP(e, hipEventCreate(ev.put()));
      e->ev_sets.push_back(std::move(set));
    }
    evs = &e->ev_sets[e->ev_used++];
  }
  auto mark = [&](int k) {  // (k: the mark before stage k of the JPEG sequence, kStageNames[k])
    if (evs) (void)hipEventRecord((*evs)[k < kPngEvent ? k : k + 2].get(), s);
    if (after_spec && (e->lane_mid == k || (e->lane_mid < 0 && k == kMarkAfterSpec))) (void)hipEventRecord(after_spec, s);
  };
  mark(0);
  SDSJ_HIP(e, launch_parse(n, d_blob, blob_bytes, d_offsets, d_lengths, op, e->warm_bits, small, ln.descs, ln.tables, s,
                           e->formats));
  if ((e->formats & SDSJ_FORMAT_PNG) && (e->formats & SDSJ_FORMAT_PNG_META))  // (counts under "parse")
    SDSJ_HIP(e, launch_png_meta(n, ln.descs, d_blob, d_offsets, d_lengths, s, e->formats));
  mark(1);
  const int cap = e->max_batch;
  SDSJ_HIP(e, launch_plan(n, ln.descs, e->capacity(), ln.base, ln.total, ln.routes, cap, s));
  if (rc_lane >= 0) {
    SDSJ_HIP(e, hipMemcpyAsync(e->h_rcounts.get() + rc_lane * kNumRoutes, ln.routes, sizeof(int32_t) * kNumRoutes,
                               hipMemcpyDeviceToHost, s));
    if (hl)  // (what k_enthint left the speculative pass in this lane's previous call: its list is reset below)
      SDSJ_HIP(e, hipMemcpyAsync(e->h_rcounts.get() + kMaxLanes * kNumRoutes + rc_lane, hl->lane, sizeof(int32_t),
                                 hipMemcpyDeviceToHost, s));
    SDSJ_HIP(e, hipEventRecord(e->ev_rc[rc_lane].get(), s));
  }
  mark(2);
  SDSJ_HIP(e, launch_unstuff(n, d_blob, d_offsets, ln.descs, e->scratch.get(), ln.routes, cap, s, rm, hint));
  SDSJ_HIP(e, launch_scanmap(n, d_blob, d_offsets, ln.descs, e->scratch.get(), s));
  mark(3);
  // (after mark 3: the next lane may start while this lane's progressive images decode)
  SDSJ_HIP(e, launch_prog(n, ln.descs, ln.tables, d_blob, d_offsets, d_lengths, e->scratch.get(), ln.routes, cap, s, rm, hint));
  if (e->formats & (SDSJ_FORMAT_JPEG_SCANS | SDSJ_FORMAT_JPEG_CMYK))  // (counts under the progressive stage)
    SDSJ_HIP(e, launch_scans(n, ln.descs, ln.tables, d_blob, d_offsets, d_lengths, e->scratch.get(), ln.routes, cap, s, rm, hint));
  if (e->formats & SDSJ_FORMAT_JPEG_CMYK_PROG)  // (progressive files of four components: likewise under "prog")
    SDSJ_HIP(e, launch_prog4(n, ln.descs, ln.tables, d_blob, d_offsets, d_lengths, e->scratch.get(), ln.routes, cap, s, rm, hint));
  if (evs) (void)hipEventRecord((*evs)[kPngEvent].get(), s);
  if (e->formats & SDSJ_FORMAT_GIF)  // (counts under "png_inflate")
    SDSJ_HIP(e, launch_gif(n, ln.descs, d_blob, d_offsets, d_lengths, e->scratch.get(), ln.routes, cap, s, rm, hint));
  if (e->formats & SDSJ_FORMAT_WEBP)  // (likewise under "png_inflate")
    SDSJ_HIP(e, launch_webp(n, ln.descs, d_blob, d_offsets, d_lengths, e->scratch.get(), ln.routes, cap, s, rm, hint));
  if (e->formats & SDSJ_FORMAT_TIFF)  // (likewise)
    SDSJ_HIP(e, launch_tiff(n, ln.descs, d_blob, d_offsets, d_lengths, e->scratch.get(), ln.routes, cap, s, rm, hint));
  if (e->formats & SDSJ_FORMAT_PNG)
    SDSJ_HIP(e, launch_png(n, ln.descs, d_blob, d_offsets, d_lengths, e->scratch.get(), ln.routes, cap, s, rm, hint,
                           evs ? (*evs)[kPngEvent + 1].get() : nullptr, e->formats));
  else if (evs)
    (void)hipEventRecord((*evs)[kPngEvent + 1].get(), s);
  mark(4);
  SDSJ_HIP(e, launch_entspec(n, ln.descs, ln.tables, ln.etab, e->scratch.get(), ln.routes, cap, s, rm, small, hint, hl));
  mark(5);
  SDSJ_HIP(e, launch_entsync(n, ln.descs, ln.etab, e->scratch.get(), ln.routes, cap, s, rm, hint, hl));
  mark(6);
  SDSJ_HIP(e, launch_entwrite(n, ln.descs, ln.etab, e->scratch.get(), ln.routes, cap, s, rm, hint, small, hl));
  mark(7);
  SDSJ_HIP(e, launch_idct(n, ln.descs, ln.tables, e->scratch.get(), s));
  if (e->formats & SDSJ_FORMAT_JPEG_CMYK)  // (four-component images: k_idct<kMaxComp> leaves them to k_idct<4>)
    SDSJ_HIP(e, launch_idct4(n, ln.descs, ln.tables, e->scratch.get(), s, rm));
  mark(8);
  SDSJ_HIP(e, launch_color(n, ln.descs, e->scratch.get(), ln.routes, cap, s, rm));
  if (e->formats & SDSJ_FORMAT_JPEG_CMYK)  // (... and k_color to k_cmyk)
    SDSJ_HIP(e, launch_cmyk(kRtScans, n, ln.descs, e->scratch.get(), ln.routes, cap, s, rm, hint));
  if (e->formats & SDSJ_FORMAT_JPEG_CMYK_PROG)  // (the progressive ones have a list of their own)
    SDSJ_HIP(e, launch_cmyk(kRtProg4, n, ln.descs, e->scratch.get(), ln.routes, cap, s, rm, hint));
  mark(9);
  SDSJ_HIP(e, launch_coeffs(n, ln.descs, op, e->scratch.get(), s));
  mark(10);
  SDSJ_HIP(e, launch_hpass(n, ln.descs, op, e->scratch.get(), ln.routes, cap, s, rm));
  mark(11);
  SDSJ_HIP(e, launch_vpass(n, ln.descs, op, e->scratch.get(), d_flip, d_out, ln.routes, cap, e->d_lut.get(), s, rm));
  mark(12);
  SDSJ_HIP(e, launch_resample(n, ln.descs, op, e->scratch.get(), d_flip, d_out, d_status, ln.routes, cap, e->d_lut.get(), s, rm, hint));
  SDSJ_HIP(e, launch_finish(n, ln.descs, op, d_out, d_status, e->d_lut.get(), d_lengths, e->d_counters.get(), s));
  mark(13);
  return SDSJ_OK;
}

// Runs one chunk (n <= max_batch).  A chunk of at least L x kLaneMin images runs as L lanes
// (contiguous image ranges) on L streams, lane k + 1 starting once lane k has planned its scratch:
// the lanes' kernel sequences overlap, so the latency-bound kernels of one lane (the entropy sync
// pass, every kernel's tail) run beside the throughput-bound kernels of another.  The caller's
// stream waits for every lane at the end.  Scratch is taken by the lanes in image order (lane k + 1's
// k_plan starts from lane k's total), so per-image results and capacity failures are those of a
// single lane.
constexpr int kLaneMin = 128;

uint64_t op_key(const sdsj_op& op) {
  return (uint64_t)(uint32_t)op.out_h | (uint64_t)(uint32_t)op.out_w << 16 | (uint64_t)(op.crop_before_resize != 0) << 32 |
         (uint64_t)(op.filter & 0xff) << 33 | (uint64_t)(op.out_dtype & 0xf) << 41 | (uint64_t)(op.layout & 0xf) << 45 |
         1ull << 63;  // (never 0: an empty slot's key)
}

uint64_t hint_lookup(const sdsj_engine* e, uint64_t key) {
  for (int k = 0; k < e->hint_n; k++)
    if (e->hint_key[k] == key) return e->hint[k];
  return kAllRoutes;
}

void hint_store(sdsj_engine* e, uint64_t key, uint64_t h) {
  for (int k = 0; k < e->hint_n; k++)
    if (e->hint_key[k] == key) {
      e->hint[k] = h;
      return;
    }
  int k = e->hint_n < sdsj_engine::kHintSlots ? e->hint_n++ : (e->hint_next++ % sdsj_engine::kHintSlots);
  e->hint_key[k] = key;
  e->hint[k] = h;
}

// rm: the routes the chunk's images may take (host planning), or kAllRoutes; small: the chunk was
// host-planned in latency mode (host paths, n <= kSmallBatch)
int run_chunk(sdsj_engine* e, int n, const uint8_t* d_blob, int64_t blob_bytes, const int64_t* d_offsets, const int32_t* d_lengths,
              const sdsj_op& op, const uint8_t* d_flip, void* d_out, int32_t* d_status, hipStream_t s,
              uint64_t rm = kAllRoutes, bool small = false, bool hints = false) {
  int nl = std::min(std::max(e->lanes, 1), kMaxLanes);
  while (nl > 1 && n < nl * kLaneMin) nl--;
  // route hint: the host paths know their routes exactly (rm); the device path uses the routes that held
  // images in the last batch of the same op whose counts have come back (all routes until one has, or
  // when the op changed: another output size selects other resample routes), and requests a new
  // readback when none is outstanding
  uint64_t hint = rm;
  bool readback = false;
  const uint64_t key = op_key(op);
  if (rm == kAllRoutes) {
    if (e->rc_pending) {
      bool done = true, lost = false;
      for (int k = 0; k < e->rc_lanes; k++) {
        const hipError_t q = hipEventQuery(e->ev_rc[k].get());
        if (q == hipErrorNotReady) done = false;
        else if (q != hipSuccess) lost = true;
      }
      if (lost) {  // a failed query: drop this readback rather than wait on it forever
        (void)hipGetLastError();
        e->rc_pending = false;
      } else if (done) {
        uint64_t h = 0;
        for (int k = 0; k < e->rc_lanes; k++)
          for (int r = 0; r < kNumRoutes; r++)
            if (e->h_rcounts.get()[k * kNumRoutes + r] > 0) h |= 1ull << r;
        if (h & (1ull << kRtEnt11M)) h |= 1ull << kRtEnt11G;
        for (int k = 0; k < e->rc_lanes; k++)  // (with the store off the bit is never read)
          if (e->h_rcounts.get()[kMaxLanes * kNumRoutes + k] != 0) h |= 1ull << kRtHintMiss;
        hint_store(e, e->rc_key, h);
        e->rc_pending = false;
      }
    }
    hint = hint_lookup(e, key);
    readback = !e->rc_pending;
  }
  const Lane first{e->descs.get(), e->tables.get(), e->d_etab.get(), e->d_routes.get(), e->d_total.get(), nullptr};
  auto readback_queued = [&](int lanes) {  // every lane recorded its ev_rc: the next call may fold them
    if (!readback) return;
    e->rc_pending = true;
    e->rc_lanes = lanes;
    e->rc_key = key;
  };
  // the entry-point store serves the device path's throughput plan (the host paths' staging addresses mean nothing)
  hints = hints && !small && e->d_hint_keys;
  const size_t hli = (size_t)hint_lane_ints(e->max_batch);
  auto hint_lane = [&](int k, int i0) {
    return HintLane{HintStore{e->d_hint_keys.get(), e->d_hint_ridx.get(), e->d_hint_ridx.get() + 2 * e->hint_rows,
                              e->d_hint_recs.get(), e->hint_rows},
                    e->d_hint_lanes.get() + k * hli,
                    e->d_hint_ctr.get(), d_blob, d_offsets + i0, d_lengths + i0};
  };
  if (nl == 1) {
    const HintLane hl = hint_lane(0, 0);
    const int st = run_lane(e, first, n, small, d_blob, blob_bytes, d_offsets, d_lengths, op, d_flip, d_out, d_status, s,
                            nullptr, rm, hint, readback ? 0 : -1, hints ? &hl : nullptr);
    if (st == SDSJ_OK) readback_queued(1);
    return st;
  }
  for (int k = 0; k + 1 < nl; k++)
    if (!e->ev_join[k]) {
      SDSJ_HIP(e, hipStreamCreateWithFlags(e->aux[k].put(), hipStreamNonBlocking));
      SDSJ_HIP(e, hipEventCreateWithFlags(e->ev_mid[k].put(), hipEventDisableTiming));
      SDSJ_HIP(e, hipEventCreateWithFlags(e->ev_join[k].put(), hipEventDisableTiming));
    }
  const int64_t ob = out_bytes_per_image(op);
  const size_t rsz = (size_t)route_ints(e->max_batch);
  for (int k = 0; k < nl; k++) {
    const int i0 = (int)((int64_t)n * k / nl), i1 = (int)((int64_t)n * (k + 1) / nl);
    const Lane ln = k == 0 ? first
                           : Lane{e->descs.get() + i0, e->tables.get() + i0,
                                  static_cast<uint8_t*>(e->d_etab.get()) + (size_t)i0 * enttab_bytes(),
                                  e->d_routes_x.get() + (k - 1) * rsz, e->d_totals_x.get() + (k - 1),
                                  k == 1 ? e->d_total.get() : e->d_totals_x.get() + (k - 2)};
    hipStream_t ls = k == 0 ? s : e->aux[k - 1].get();
    if (k > 0) SDSJ_HIP(e, hipStreamWaitEvent(ls, e->ev_mid[k - 1].get(), 0));
    const HintLane hl = hint_lane(k, i0);
    int st = run_lane(e, ln, i1 - i0, small, d_blob, blob_bytes, d_offsets + i0, d_lengths + i0, op, d_flip ? d_flip + i0 : nullptr,
                      static_cast<uint8_t*>(d_out) + i0 * ob, d_status + i0, ls,
                      k + 1 < nl ? e->ev_mid[k].get() : nullptr, rm, hint, readback ? k : -1, hints ? &hl : nullptr);
    if (st != SDSJ_OK) return st;
  }
  readback_queued(nl);
  for (int k = 0; k + 1 < nl; k++) {
    SDSJ_HIP(e, hipEventRecord(e->ev_join[k].get(), e->aux[k].get()));
    SDSJ_HIP(e, hipStreamWaitEvent(s, e->ev_join[k].get(), 0));
  }
  return SDSJ_OK;
}

// -- host paths (sdsj_decode_resize_batch, sdsj_submit_*) --------------------------------------
// Each is reserve + stage (stage_batch), plan + launch (stage_launch) and wait + merge
// (stage_collect) on a Staging: the engine's `sync_stage` one chunk at a time, or a slot.

// Host staging (copies / file reads into pinned memory, header planning) is split over threads:
// a single core's memcpy bandwidth would otherwise bound the pipelined host path.
int stage_threads() {
  static const int k = [] {
    const char* v = getenv("SDSJ_STAGE_THREADS");
    const int hw = (int)std::thread::hardware_concurrency();
    const int d = std::max(1, std::min(8, hw > 0 ? hw : 1));
    return v ? std::max(1, atoi(v)) : d;
  }();
  return k;
}

// Serial below 32 samples: small calls start no threads.
template <class F>
void parallel_for(sdsj_engine* e, int n, F fn) {
  const int nt = std::min(stage_threads(), std::max(1, n / 16));
  if (nt <= 1) {
    fn(0, n);
    return;
  }
  if (!e->pool) e->pool.reset(new StagePool(stage_threads() - 1));
  e->pool->parallel_for(n, nt, fn);
}

// Waits for the staging's batch in flight, if any: its pinned and device buffers are then free.
int stage_wait(sdsj_engine* e, Staging& st) {
  if (!st.pending) return SDSJ_OK;
  if (st.ev_done) SDSJ_HIP(e, hipEventSynchronize(st.ev_done.get()));
  else SDSJ_HIP(e, hipStreamSynchronize(st.stream));
  st.pending = false;
  return SDSJ_OK;
}

// Waits for the staging's previous use and sizes it for n samples in a region of `total` bytes.
int stage_reserve(sdsj_engine* e, Staging& st, int n, int64_t total) {
  const int rc = stage_wait(e, st);
  if (rc != SDSJ_OK) return rc;
  if (n > st.cap) {
    const int cap = std::max(n, 64);
    st.cap = 0;
    if (!st.h_status.reserve(cap) || !st.d_status.reserve(cap)) return alloc_fail(e, "status allocation");
    st.pre.reset(new (std::nothrow) int32_t[cap]);
    if (!st.pre) return fail(e, SDSJ_ENOMEM, "host allocation failed");
    st.cap = cap;
  }
  if ((size_t)total > st.d.size()) {
    const size_t cap = std::max<size_t>((size_t)total * 3 / 2, 1 << 20);
    st.d.reset();  // (the check above reads d: empty unless both were allocated)
    if (!st.h.reserve(cap) || !st.d.reserve(cap)) return alloc_fail(e, "staging allocation");
  }
  return SDSJ_OK;
}

// Reserves the staging and fills its pinned region with n samples: size(i) is sample i's byte count
// (< 0: unreadable) and fill(i, dst) writes it, false on failure.  A sample that failed has length -1 on
// the device (k_finish reports a negative length as EINVAL, counted "other") and SDSJ_EINVAL in `pre`.
template <class Size, class Fill>
int stage_batch(sdsj_engine* e, Staging& st, int n, const uint8_t* flip, Size size, Fill fill) {
  int64_t bytes = 0;
  for (int i = 0; i < n; i++)
    if (size(i) > 0) bytes += align_up(size(i), 16);
  const StageLayout lay = stage_layout(n, bytes);
  const int rc = stage_reserve(e, st, n, lay.total);
  if (rc != SDSJ_OK) return rc;
  st.lay = lay;
  st.n = n;
  int64_t off = 0;
  for (int i = 0; i < n; i++) {
    st.offsets()[i] = off;
    st.flip()[i] = flip ? flip[i] : 0;
    if (size(i) > 0) off += align_up(size(i), 16);
  }
  parallel_for(e, n, [&](int i0, int i1) {
    for (int i = i0; i < i1; i++) {
      const bool ok = size(i) >= 0 && fill(i, st.h.get() + st.offsets()[i]);
      st.lengths()[i] = ok ? (int32_t)size(i) : -1;
      st.pre[i] = ok ? SDSJ_OK : SDSJ_EINVAL;
    }
  });
  return SDSJ_OK;
}

// The staged batch (n > 0): scratch sized from host planning over the pinned copy, the region's one H2D
// on `cs`, the decode on `s` (behind that copy through ev_h2d when cs is another stream), status D2H
// into pinned memory, and the completion event where the staging has one.
int stage_launch(sdsj_engine* e, Staging& st, const sdsj_op& op, void* out, hipStream_t s, hipStream_t cs) {
  const int n = st.n;
  const bool small = n <= kSmallBatch;
  std::vector<int64_t> needs(n, 0);
  std::atomic<uint64_t> rmask{0};  // the routes the batch takes (launchers skip the others)
  parallel_for(e, n, [&](int i0, int i1) {
    uint64_t rm = 0;
    for (int i = i0; i < i1; i++) {
      if (st.pre[i] != SDSJ_OK) continue;
      int ist = SDSJ_OK;
      uint64_t r = 0;
      const int64_t ni = host_plan_need(st.h.get() + st.offsets()[i], st.lengths()[i], op, &ist, &r, small, e->formats);
      if (ist == SDSJ_OK) needs[i] = align_up(ni, 256);
      rm |= r;
    }
    rmask.fetch_or(rm);
  });
  int64_t need = 0;
  for (int i = 0; i < n; i++) need += needs[i];
  int rc = scratch_for(e, need, s, "batch exceeds the configured scratch capacity");
  if (rc != SDSJ_OK) return rc;
  const StageLayout& lay = st.lay;
  uint8_t* d = st.d.get();
  SDSJ_HIP(e, hipMemcpyAsync(d, st.h.get(), (size_t)lay.total, hipMemcpyHostToDevice, cs));
  if (cs != s) {
    SDSJ_HIP(e, hipEventRecord(st.ev_h2d.get(), cs));
    SDSJ_HIP(e, hipStreamWaitEvent(s, st.ev_h2d.get(), 0));
  }
  // (blob_bytes = lay.offsets, the end of the sample region: the metadata behind it is no sample)
  rc = run_chunk(e, n, d, lay.offsets, reinterpret_cast<const int64_t*>(d + lay.offsets),
                 reinterpret_cast<const int32_t*>(d + lay.lengths), op, d + lay.flip, out, st.d_status.get(), s,
                 rmask.load(), small);
  if (rc != SDSJ_OK) return rc;
  SDSJ_HIP(e, hipMemcpyAsync(st.h_status.get(), st.d_status.get(), sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
  if (st.ev_done) SDSJ_HIP(e, hipEventRecord(st.ev_done.get(), s));
  st.stream = s;
  st.pending = true;
  return SDSJ_OK;
}

// Waits for the staging's batch and merges the host pre-status into the device's statuses.
int stage_collect(sdsj_engine* e, Staging& st, int32_t* status) {
  const int rc = stage_wait(e, st);
  if (rc != SDSJ_OK) return rc;
  if (status)
    for (int i = 0; i < st.n; i++) status[i] = st.pre[i] != SDSJ_OK ? st.pre[i] : st.h_status.get()[i];
  return SDSJ_OK;
}

// A slot's copy stream and events, created on its first use.
int slot_setup(sdsj_engine* e, Staging& sl) {
  if (!e->copy_stream) SDSJ_HIP(e, hipStreamCreateWithFlags(e->copy_stream.put(), hipStreamNonBlocking));
  if (!sl.ev_done) {
    SDSJ_HIP(e, hipEventCreateWithFlags(sl.ev_h2d.put(), hipEventDisableTiming));
    SDSJ_HIP(e, hipEventCreateWithFlags(sl.ev_done.put(), hipEventDisableTiming));
  }
  return SDSJ_OK;
}

// Launches a slot's staged batch; an empty one still marks the slot pending and records its event.
int slot_launch(sdsj_engine* e, Staging& sl, const sdsj_op& op, void* out, hipStream_t s) {
  if (sl.n > 0) return stage_launch(e, sl, op, out, s, e->copy_stream.get());
  sl.stream = s;
  sl.pending = true;
  return hipEventRecord(sl.ev_done.get(), s) == hipSuccess ? SDSJ_OK : SDSJ_EHIP;
}

int64_t file_size(const char* path) {
  struct stat sb;
  if (!path || stat(path, &sb) != 0 || !S_ISREG(sb.st_mode)) return -1;
  return (int64_t)sb.st_size;
}

// Reads exactly `size` bytes of `path` into dst; false on any error or a short file.
bool read_file(const char* path, uint8_t* dst, int64_t size) {
  const int fd = open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) return false;
  int64_t got = 0;
  while (got < size) {
    const ssize_t r = read(fd, dst + got, (size_t)std::min<int64_t>(size - got, 1 << 30));
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) break;
    got += r;
  }
  close(fd);
  return got == size;
}

// The engine's fixed allocations: SDSJ_ENOMEM for a failed allocation, SDSJ_EHIP for a failed event,
// memset or memcpy.
int engine_init(sdsj_engine* e, const sdsj_cfg* cfg) {
  if (const char* w = getenv("SDSJ_WARM_BITS")) e->warm_bits = atoi(w);
  if (cfg && cfg->max_batch > 0) e->max_batch = cfg->max_batch;
  if (const char* l = getenv("SDSJ_LANES")) e->lanes = atoi(l);
  if (const char* l = getenv("SDSJ_LANE_MID")) e->lane_mid = atoi(l);
  if (e->lane_mid >= 0 && e->lane_mid < 2) e->lane_mid = 2;  // a lane's k_plan reads the previous lane's total
  const size_t mb = (size_t)e->max_batch, routes = (size_t)route_ints(e->max_batch);
  if (!e->descs.reserve(mb) || !e->tables.reserve(mb) || !e->d_total.reserve(1) || !e->d_totals_x.reserve(kMaxLanes - 1) ||
      !e->d_routes_x.reserve((kMaxLanes - 1) * routes) || !e->d_etab.reserve(enttab_bytes() * mb) ||
      !e->d_routes.reserve(routes) || !e->d_lut.reserve(256) || !e->h_rcounts.reserve(kMaxLanes * (kNumRoutes + 1)) ||
      !e->d_counters.reserve(SDSJ_NUM_COUNTERS) || !e->d_hint_ctr.reserve(SDSJ_NUM_HINT_COUNTERS))
    return SDSJ_ENOMEM;
  if (const char* h = getenv("SDSJ_HINTS"))
    if (atoi(h) == 0) e->hint_rows = 0;
  if (e->hint_rows < 0) e->hint_rows = 2 * (int64_t)e->max_batch;
  for (int k = 0; k < kMaxLanes * (kNumRoutes + 1); k++) e->h_rcounts.get()[k] = 0;
  if (hipMemset(e->d_hint_ctr.get(), 0, sizeof(unsigned long long) * SDSJ_NUM_HINT_COUNTERS) != hipSuccess) return SDSJ_EHIP;
  for (auto& ev : e->ev_rc)
    if (hipEventCreateWithFlags(ev.put(), hipEventDisableTiming) != hipSuccess) return SDSJ_EHIP;
  if (hipMemset(e->d_counters.get(), 0, sizeof(unsigned long long) * SDSJ_NUM_COUNTERS) != hipSuccess) return SDSJ_EHIP;
  // presets.py:161 `x.float() / 127.5 - 1.0` in float32 (IEEE division then subtraction)
  float lut[256];
  volatile float div = 127.5f, one = 1.0f;
  for (int v = 0; v < 256; v++) {
    float q = (float)v / div;
    lut[v] = q - one;
  }
  if (hipMemcpy(e->d_lut.get(), lut, sizeof(lut), hipMemcpyHostToDevice) != hipSuccess) return SDSJ_EHIP;
  if (cfg && cfg->scratch_bytes > 0) {
    e->grow = false;
    return ensure_scratch(e, cfg->scratch_bytes);
  }
  return SDSJ_OK;
}

// Every key slot free, no record handed out.  (The caller has waited for the device.)
int hints_empty(sdsj_engine* e) {
  const size_t slots = 2 * (size_t)e->hint_rows;
  SDSJ_HIP(e, hipMemset(e->d_hint_keys.get(), 0, sizeof(unsigned long long) * slots));
  SDSJ_HIP(e, hipMemset(e->d_hint_ridx.get(), 0, sizeof(int32_t) * (slots + 1)));
  return SDSJ_OK;
}

// The entry-point store's memory, on the first device-resident call that may use it.  A store that cannot be
// allocated is a store turned off: the call decodes the ordinary way.
int ensure_hints(sdsj_engine* e) {
  if (e->hint_rows <= 0 || e->d_hint_keys) return SDSJ_OK;
  const size_t lanes = (size_t)kMaxLanes * (size_t)hint_lane_ints(e->max_batch);
  const size_t slots = 2 * (size_t)e->hint_rows;
  if (!e->d_hint_recs.reserve((size_t)e->hint_rows * kHintRowBytes) || !e->d_hint_lanes.reserve(lanes) ||
      !e->d_hint_ridx.reserve(slots + 1) || !e->d_hint_keys.reserve(slots)) {
    (void)hipGetLastError();
    e->d_hint_keys.reset();
    e->d_hint_ridx.reset();
    e->d_hint_recs.reset();
    e->hint_rows = 0;
    return SDSJ_OK;
  }
  SDSJ_HIP(e, hipMemset(e->d_hint_lanes.get(), 0, sizeof(int32_t) * lanes));
  return hints_empty(e);
}

// An emptied store (or another size) makes every row a miss: the speculative pass gets its full grid again.
void hints_forget(sdsj_engine* e) {
  for (int k = 0; k < e->hint_n; k++) e->hint[k] |= 1ull << kRtHintMiss;
}
}  // namespace

extern "C" {

int sdsj_abi_version(void) { return SDSJ_ABI_VERSION; }

int sdsj_submit_batch(sdsj_engine* e, int slot, int n, const uint8_t* const* jpg, const size_t* len, const sdsj_op* op,
                      const uint8_t* flip, void* out, void* hip_stream) {
  if (!e) return SDSJ_EINVAL;
  if (slot < 0 || slot >= SDSJ_SLOTS || n < 0 || n > e->max_batch || (n > 0 && (!jpg || !len || !out)) ||
      !valid_op(op))
    return fail(e, SDSJ_EINVAL, "invalid argument");
  DeviceGuard g(e->device);
  Staging& sl = e->slots[slot];
  for (int i = 0; i < n; i++)
    if (len[i] > (size_t)INT32_MAX) return fail(e, SDSJ_EINVAL, "sample larger than 2 GiB");
  int rc = slot_setup(e, sl);
  if (rc == SDSJ_OK)
    rc = stage_batch(
        e, sl, n, flip, [&](int i) { return (int64_t)len[i]; },
        [&](int i, uint8_t* dst) {
          memcpy(dst, jpg[i], len[i]);
          return true;
        });
  if (rc != SDSJ_OK) return rc;
  return slot_launch(e, sl, *op, out, reinterpret_cast<hipStream_t>(hip_stream));
}

int sdsj_submit_files(sdsj_engine* e, int slot, int n, const char* const* paths, const sdsj_op* op,
                      const uint8_t* flip, void* out, void* hip_stream) {
  if (!e) return SDSJ_EINVAL;
  if (slot < 0 || slot >= SDSJ_SLOTS || n < 0 || n > e->max_batch || (n > 0 && (!paths || !out)) || !valid_op(op))
    return fail(e, SDSJ_EINVAL, "invalid argument");
  DeviceGuard g(e->device);
  Staging& sl = e->slots[slot];
  std::vector<int64_t> sizes(n);
  parallel_for(e, n, [&](int i0, int i1) {
    for (int i = i0; i < i1; i++) {
      sizes[i] = file_size(paths[i]);
      if (sizes[i] > INT32_MAX) sizes[i] = -1;
    }
  });
  int rc = slot_setup(e, sl);
  if (rc == SDSJ_OK)
    rc = stage_batch(
        e, sl, n, flip, [&](int i) { return sizes[i]; },
        [&](int i, uint8_t* dst) { return read_file(paths[i], dst, sizes[i]); });
  if (rc != SDSJ_OK) return rc;
  return slot_launch(e, sl, *op, out, reinterpret_cast<hipStream_t>(hip_stream));
}

int sdsj_wait_batch(sdsj_engine* e, int slot, int32_t* status) {
  if (!e) return SDSJ_EINVAL;
  if (slot < 0 || slot >= SDSJ_SLOTS || !e->slots[slot].pending) return fail(e, SDSJ_EINVAL, "no batch in flight on slot");
  DeviceGuard g(e->device);
  return stage_collect(e, e->slots[slot], status);
}

int sdsj_probe(const uint8_t* jpg, size_t n, sdsj_info* out) { return sdsj_probe_formats(jpg, n, SDSJ_FORMAT_JPEG, out); }

int sdsj_probe_formats(const uint8_t* jpg, size_t n, int formats, sdsj_info* out) {
  if (!jpg || !out || !(formats & SDSJ_FORMAT_JPEG)) return SDSJ_EINVAL;
  if ((formats & SDSJ_FORMAT_JPEG_CMYK_PROG) && !(formats & SDSJ_FORMAT_JPEG_CMYK)) return SDSJ_EINVAL;  // (valid_formats)
  memset(out, 0, sizeof(*out));
  ImgDesc d;
  static thread_local ImgTables t;
  MemReader rd{jpg};
  int st = parse_sample(rd, (int64_t)n, &d, &t, CopySink<MemReader>{rd}, formats);
  out->width = d.width;
  out->height = d.height;
  out->ncomp = d.ncomp;
  if (st == SDSJ_OK && !scan_tables_ok(d, t)) st = SDSJ_CORRUPT;
  if (st == SDSJ_OK && d.progressive == kScansSequential) st = scans_check(rd, (int64_t)n, d);
  for (int c = 0; c < d.ncomp && c < 3; c++) {
    out->h_samp[c] = d.comp[c].h;
    out->v_samp[c] = d.comp[c].v;
  }
  out->restart_interval = d.restart_interval;
  out->entropy_offset = st == SDSJ_OK ? d.entropy_off : 0;
  out->supported = st == SDSJ_OK;
  return st;
}

int sdsj_plan_need(const uint8_t* jpg, size_t n, const sdsj_op* op, int64_t* need) {
  if (!jpg || !need || !valid_op(op)) return SDSJ_EINVAL;
  int st = SDSJ_OK;
  const int64_t b = host_plan_need(jpg, (int64_t)n, *op, &st);
  *need = st == SDSJ_OK ? align_up(b, 256) : 0;
  return st;
}

// A format mask names at least one of JPEG, PNG, GIF, WEBP and TIFF, nothing unknown, PNG_EXT and PNG_META (alone or
// together) only with PNG, JPEG_EXT, JPEG_SCANS and JPEG_CMYK (in any combination) only with JPEG, and JPEG_CMYK_PROG
// only with JPEG_CMYK (and so with JPEG).
static bool valid_formats(int mask) {
  const int sub = SDSJ_FORMAT_PNG_EXT | SDSJ_FORMAT_PNG_META;
  const int jsub = SDSJ_FORMAT_JPEG_EXT | SDSJ_FORMAT_JPEG_SCANS | SDSJ_FORMAT_JPEG_CMYK | SDSJ_FORMAT_JPEG_CMYK_PROG;
  if ((mask & SDSJ_FORMAT_JPEG_CMYK_PROG) && !(mask & SDSJ_FORMAT_JPEG_CMYK)) return false;
  const int base = SDSJ_FORMAT_JPEG | SDSJ_FORMAT_PNG | SDSJ_FORMAT_GIF | SDSJ_FORMAT_WEBP | SDSJ_FORMAT_TIFF, all = base | sub | jsub;
  return (mask & base) && !(mask & ~all) && (!(mask & sub) || (mask & SDSJ_FORMAT_PNG)) &&
         (!(mask & jsub) || (mask & SDSJ_FORMAT_JPEG));
}

int sdsj_plan_need_formats(const uint8_t* img, size_t n, const sdsj_op* op, int formats, int64_t* need) {
  if (!img || !need || !valid_op(op) || !valid_formats(formats)) return SDSJ_EINVAL;
  int st = SDSJ_OK, later = SDSJ_OK;
  const int64_t b = host_plan_need(img, (int64_t)n, *op, &st, nullptr, false, formats, &later);
  *need = st == SDSJ_OK ? align_up(b, 256) : 0;
  // (a multi-scan file refused over its scans: the device plans its scratch before k_scans refuses it, so a batch
  // that holds it needs these bytes)
  return st == SDSJ_OK ? later : st;
}

int sdsj_engine_set_formats(sdsj_engine* e, int mask) {
  if (!e) return SDSJ_EINVAL;
  if (!valid_formats(mask)) return fail(e, SDSJ_EINVAL, "invalid format mask");
  e->formats = mask;
  return SDSJ_OK;
}

int sdsj_engine_create(int hip_device, const sdsj_cfg* cfg, sdsj_engine** out) {
  if (!out) return SDSJ_EINVAL;
  *out = nullptr;
  if (cfg && cfg->abi_version != SDSJ_ABI_VERSION) return SDSJ_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || hip_device < 0 || hip_device >= ndev) return SDSJ_EHIP;
  sdsj_engine* e = new (std::nothrow) sdsj_engine();
  if (!e) return SDSJ_ENOMEM;
  e->device = hip_device;
  DeviceGuard g(hip_device);
  const int st = engine_init(e, cfg);
  if (st != SDSJ_OK) {
    sdsj_engine_destroy(e);
    return st;
  }
  *out = e;
  return SDSJ_OK;
}

// Every buffer, stream and event is an owner (sdsj_buffers.h): deleting the engine releases them, with
// its device current.
int sdsj_engine_destroy(sdsj_engine* e) {
  if (!e) return SDSJ_EINVAL;
  DeviceGuard g(e->device);
  (void)hipDeviceSynchronize();
  delete e;
  return SDSJ_OK;
}

int sdsj_decode_resize_batch_device(sdsj_engine* e, int n, const uint8_t* d_blob, size_t blob_bytes,
                                    const int64_t* d_offsets, const int32_t* d_lengths, const sdsj_op* op,
                                    const uint8_t* d_flip, void* d_out, int32_t* d_status, void* hip_stream) {
  if (!e) return SDSJ_EINVAL;
  if (n < 0 || (n > 0 && (!d_blob || !d_offsets || !d_lengths || !d_out || !d_status)) || !valid_op(op))
    return fail(e, SDSJ_EINVAL, "invalid argument");
  if (n == 0) return SDSJ_OK;
  DeviceGuard g(e->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  if (!e->scratch) {
    int st = ensure_scratch(e, (int64_t)2 << 30);
    if (st != SDSJ_OK) return st;
  }
  {
    const int st = ensure_hints(e);
    if (st != SDSJ_OK) return st;
  }
  const int64_t ob = out_bytes_per_image(*op);
  for (int c0 = 0; c0 < n; c0 += e->max_batch) {
    int m = std::min(e->max_batch, n - c0);
    int st = run_chunk(e, m, d_blob, (int64_t)blob_bytes, d_offsets + c0, d_lengths + c0, *op, d_flip ? d_flip + c0 : nullptr,
                       reinterpret_cast<uint8_t*>(d_out) + c0 * ob, d_status + c0, s, kAllRoutes, false, true);
    if (st != SDSJ_OK) return st;
  }
  return SDSJ_OK;
}

int sdsj_decode_resize_batch(sdsj_engine* e, int n, const uint8_t* const* jpg, const size_t* len, const sdsj_op* op,
                             const uint8_t* flip, void* out, int32_t* status, void* hip_stream) {
  if (!e) return SDSJ_EINVAL;
  if (n < 0 || (n > 0 && (!jpg || !len || !out || !status)) || !valid_op(op))
    return fail(e, SDSJ_EINVAL, "invalid argument");
  for (int i = 0; i < n; i++)
    if (len[i] > (size_t)INT32_MAX) return fail(e, SDSJ_EINVAL, "sample larger than 2 GiB");
  if (n == 0) return SDSJ_OK;
  DeviceGuard g(e->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  const int64_t ob = out_bytes_per_image(*op);
  // one chunk at a time through the one staging, everything on the caller's stream: the H2D copy, the
  // kernels, the status copy and the wait (no event, no second stream)
  Staging& st = e->sync_stage;
  for (int c0 = 0; c0 < n; c0 += e->max_batch) {
    const int m = std::min(e->max_batch, n - c0);
    int rc = stage_batch(
        e, st, m, flip ? flip + c0 : nullptr, [&](int i) { return (int64_t)len[c0 + i]; },
        [&](int i, uint8_t* dst) {
          memcpy(dst, jpg[c0 + i], len[c0 + i]);
          return true;
        });
    if (rc == SDSJ_OK) rc = stage_launch(e, st, *op, reinterpret_cast<uint8_t*>(out) + c0 * ob, s, s);
    if (rc == SDSJ_OK) rc = stage_collect(e, st, status + c0);
    if (rc != SDSJ_OK) return rc;
  }
  return SDSJ_OK;
}

int sdsj_resize_frames_device(sdsj_engine* e, int n, const uint8_t* d_frames, int32_t width, int32_t height,
                              int64_t frame_stride, const sdsj_op* op, const uint8_t* d_flip, void* d_out,
                              int32_t* d_status, void* hip_stream) {
  if (!e) return SDSJ_EINVAL;
  if (n < 0 || (n > 0 && (!d_frames || !d_out || !d_status)) || !valid_op(op) || width <= 0 || height <= 0 ||
      width > 65535 || height > 65535 || frame_stride < (int64_t)width * height * 3)
    return fail(e, SDSJ_EINVAL, "invalid argument");
  if (n == 0) return SDSJ_OK;
  DeviceGuard g(e->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  ImgDesc base;
  const int64_t need = align_up(host_plan_frame(&base, width, height, *op), 256);
  const int cap = e->max_batch;
  if (!e->h_froutes && (!e->h_fdescs.reserve(cap) || !e->h_froutes.reserve(kRouteSlots + cap)))
    return alloc_fail(e, "frame staging allocation");
  const int64_t ob = out_bytes_per_image(*op);
  for (int c0 = 0; c0 < n; c0 += cap) {
    const int m = std::min(cap, n - c0);
    const int rc = scratch_for(e, need * m, s, "frames exceed the configured scratch capacity", (int64_t)256 << 20);
    if (rc != SDSJ_OK) return rc;
    SDSJ_HIP(e, hipStreamSynchronize(s));  // the pinned staging is reused chunk to chunk
    for (int k = 0; k < m; k++) {
      ImgDesc& d = e->h_fdescs.get()[k];
      d = base;
      const int64_t o = need * k;
      d.off_ustream += o;
      d.off_seg += o;
      d.off_tiles += o;
      d.off_sub += o;
      d.off_rec += o;
      d.off_ptab += o;
      d.off_coef += o;
      d.off_planes += o;
      d.off_tmp += o;
      d.off_kh += o;
      d.off_kv += o;
      // the passes read the frame's crop rows in place: scratch + off_rgb = the crop's first pixel
      const uint8_t* px = d_frames + (int64_t)(c0 + k) * frame_stride + ((int64_t)d.src_y0 * width + d.src_x0) * 3;
      d.off_rgb = (int64_t)(px - e->scratch.get());
      d.rgb_pitch = width;
    }
    int32_t* froutes = e->h_froutes.get();
    for (int r = 0; r < kRouteSlots; r++) froutes[r] = 0;
    froutes[kRtUnfused] = m;
    for (int k = 0; k < m; k++) froutes[kRouteSlots + kRtUnfused * cap + k] = k;
    SDSJ_HIP(e, hipMemcpyAsync(e->descs.get(), e->h_fdescs.get(), sizeof(ImgDesc) * m, hipMemcpyHostToDevice, s));
    SDSJ_HIP(e, hipMemcpyAsync(e->d_routes.get(), froutes, sizeof(int32_t) * (kRouteSlots + m), hipMemcpyHostToDevice, s));
    void* out = reinterpret_cast<uint8_t*>(d_out) + c0 * ob;
    const uint8_t* flip = d_flip ? d_flip + c0 : nullptr;
    SDSJ_HIP(e, launch_coeffs(m, e->descs.get(), *op, e->scratch.get(), s));
    SDSJ_HIP(e, launch_hpass(m, e->descs.get(), *op, e->scratch.get(), e->d_routes.get(), cap, s));
    SDSJ_HIP(e, launch_vpass(m, e->descs.get(), *op, e->scratch.get(), flip, out, e->d_routes.get(), cap, e->d_lut.get(), s));
    SDSJ_HIP(e, launch_finish(m, e->descs.get(), *op, out, d_status + c0, e->d_lut.get(), nullptr, e->d_counters.get(), s));
  }
  return SDSJ_OK;
}

int sdsj_engine_set_timing(sdsj_engine* e, int enable) {
  if (!e) return SDSJ_EINVAL;
  e->timing = enable != 0;
  e->ev_used = 0;  // restart accumulation
  return SDSJ_OK;
}

int sdsj_engine_stage_times(const sdsj_engine* e, float* ms, int cap, int* n_stages) {
  if (!e || !n_stages || (cap > 0 && !ms)) return SDSJ_EINVAL;
  *n_stages = kStages;
  for (int k = 0; k < cap && k < kStages; k++) ms[k] = 0.f;
  if (!e->timing || e->ev_used == 0) return SDSJ_OK;
  DeviceGuard g(e->device);
  for (size_t c = 0; c < e->ev_used; c++)  // lanes run on two streams: wait for every set
    if (hipEventSynchronize(e->ev_sets[c][kStages].get()) != hipSuccess) return SDSJ_EHIP;
  for (size_t c = 0; c < e->ev_used; c++) {
    for (int k = 0; k < cap && k < kStages; k++) {
      float v = 0.f;
      const int ev = stage_event(k);
      if (hipEventElapsedTime(&v, e->ev_sets[c][ev].get(), e->ev_sets[c][ev + 1].get()) != hipSuccess) return SDSJ_EHIP;
      ms[k] += v;
    }
  }
  return SDSJ_OK;
}

const char* sdsj_last_error(const sdsj_engine* e) {
  if (!e) return "null engine";
  return e->err.c_str();
}

int sdsj_engine_debug_buffers(const sdsj_engine* e, void** scratch, void** descs, int64_t* desc_bytes,
                              int64_t* scratch_bytes) {
  if (!e || !scratch || !descs || !desc_bytes || !scratch_bytes) return SDSJ_EINVAL;
  *scratch = e->scratch.get();
  *descs = e->descs.get();
  *desc_bytes = (int64_t)sizeof(ImgDesc);
  *scratch_bytes = e->capacity();
  return SDSJ_OK;
}

const char* sdsj_stage_name(int k) { return k >= 0 && k < kStages ? kStageNames[k] : ""; }

int sdsj_engine_counters(sdsj_engine* e, uint64_t* out, int cap, int reset) {
  if (!e || (cap > 0 && !out)) return SDSJ_EINVAL;
  DeviceGuard g(e->device);
  unsigned long long h[SDSJ_NUM_COUNTERS];
  SDSJ_HIP(e, hipDeviceSynchronize());
  SDSJ_HIP(e, hipMemcpy(h, e->d_counters.get(), sizeof(h), hipMemcpyDeviceToHost));
  for (int k = 0; k < cap && k < SDSJ_NUM_COUNTERS; k++) out[k] = (uint64_t)h[k];
  if (reset) {
    SDSJ_HIP(e, hipMemset(e->d_counters.get(), 0, sizeof(h)));
  }
  return SDSJ_OK;
}

const char* sdsj_counter_name(int k) {
  static const char* names[SDSJ_NUM_COUNTERS] = {"images",    "ok",        "unsupported", "corrupt", "capacity",
                                                 "other",     "bytes_in",  "bytes_out",   "frames",  "progressive",
                                                 "png"};
  return k >= 0 && k < SDSJ_NUM_COUNTERS ? names[k] : "";
}

int sdsj_engine_set_hints(sdsj_engine* e, int64_t rows) {
  if (!e || rows < 0) return SDSJ_EINVAL;
  DeviceGuard g(e->device);
  SDSJ_HIP(e, hipDeviceSynchronize());
  e->d_hint_keys.reset();
  e->d_hint_ridx.reset();
  e->d_hint_recs.reset();
  e->hint_rows = rows;  // (allocated by the next device-resident call)
  hints_forget(e);
  return SDSJ_OK;
}

int sdsj_engine_clear_hints(sdsj_engine* e) {
  if (!e) return SDSJ_EINVAL;
  if (!e->d_hint_keys) return SDSJ_OK;
  DeviceGuard g(e->device);
  SDSJ_HIP(e, hipDeviceSynchronize());
  const int st = hints_empty(e);
  hints_forget(e);
  return st;
}

int sdsj_engine_hint_counters(sdsj_engine* e, uint64_t* out, int cap, int reset) {
  if (!e || (cap > 0 && !out)) return SDSJ_EINVAL;
  DeviceGuard g(e->device);
  unsigned long long h[SDSJ_NUM_HINT_COUNTERS];
  SDSJ_HIP(e, hipDeviceSynchronize());
  SDSJ_HIP(e, hipMemcpy(h, e->d_hint_ctr.get(), sizeof(h), hipMemcpyDeviceToHost));
  for (int k = 0; k < cap && k < SDSJ_NUM_HINT_COUNTERS; k++) out[k] = (uint64_t)h[k];
  if (reset) SDSJ_HIP(e, hipMemset(e->d_hint_ctr.get(), 0, sizeof(h)));
  return SDSJ_OK;
}

const char* sdsj_hint_counter_name(int k) {
  static const char* names[SDSJ_NUM_HINT_COUNTERS] = {"hint_hits", "hint_misses", "hint_verify_failed", "hint_stored"};
  return k >= 0 && k < SDSJ_NUM_HINT_COUNTERS ? names[k] : "";
}

int sdsj_engine_set_lanes(sdsj_engine* e, int lanes) {
  if (!e || lanes < 1 || lanes > kMaxLanes) return SDSJ_EINVAL;
  e->lanes = lanes;
  return SDSJ_OK;
}

int sdsj_engine_reserve(sdsj_engine* e, int64_t bytes) {
  if (!e || bytes < 0) return SDSJ_EINVAL;
  DeviceGuard g(e->device);
  if (bytes <= e->capacity() && e->scratch) return SDSJ_OK;
  SDSJ_HIP(e, hipDeviceSynchronize());
  return ensure_scratch(e, bytes);
}

}  // extern "C"
