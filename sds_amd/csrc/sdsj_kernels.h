// sdsj_kernels.h -- launchers of every stage file's gfx950 kernels (sdsj_plan.hip, sdsj_unstuff.hip,
// sdsj_entropy.hip, sdsj_progressive.hip, sdsj_scans.hip, sdsj_png.hip, sdsj_png_ext.hip, sdsj_idct.hip, sdsj_unfused.hip, sdsj_resample.hip,
// sdsj_resample420.hip) and host-side planning (sdsj_plan.hip); engine-internal.
#pragma once
#include <hip/hip_runtime.h>

#include "sdsj_common.h"

namespace sdsj {
// Route masks (bit r = route r may hold images): launchers skip the variant kernels of routes whose
// bit is clear.  The host paths know every image's routes from host planning (host_plan_need); the
// device-resident path passes kAllRoutes (its route lists exist only on the device).
constexpr uint64_t kAllRoutes = ~0ull;
SDSJ_HD inline bool route_on(uint64_t rm, int r) { return (rm >> r) & 1ull; }
// Route hints (hint: bit r = route r held images in a recent batch of this engine): a launched route
// outside the hint gets a small grid whose workgroups stride over its list -- exact for any count,
// only slower -- instead of one workgroup per possible entry.  The device path launches every route
// (its lists exist only on the device), and most of them are empty for a given dataset: thousands
// of empty workgroups per launch otherwise (sdsj_engine.hip run_chunk keeps the hint).
constexpr int kColdGrid = 64;
inline unsigned route_grid(uint64_t hint, int r, int64_t full) {
  return (unsigned)(route_on(hint, r) || full < kColdGrid ? full : kColdGrid);
}
// blob_bytes: the blob's size -- a sample whose [offset, offset + length) leaves it is reported EINVAL
// formats: SDSJ_FORMAT_* mask of the engine (samples of a format outside it report SDSJ_UNSUPPORTED)
hipError_t launch_parse(int n, const uint8_t* blob, int64_t blob_bytes, const int64_t* offsets, const int32_t* lengths,
                        const sdsj_op& op, int warm_bits, bool small, ImgDesc* descs, ImgTables* tables, hipStream_t s,
                        int formats = SDSJ_FORMAT_JPEG);
// PNG samples (route kRtPng): k_png_inflate then k_png_unfilter (sdsj_png.hip) and, when `formats` has
// SDSJ_FORMAT_PNG_EXT, k_png_unfilter_ext (sdsj_png_ext.hip); `between` (optional) is
// recorded between the two
hipError_t launch_png(int n, ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, const int32_t* lengths,
                      uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s, uint64_t rm = kAllRoutes,
                      uint64_t hint = kAllRoutes, hipEvent_t between = nullptr, int formats = SDSJ_FORMAT_PNG);
// GIF samples (route kRtGif; engines with SDSJ_FORMAT_GIF): k_gif_lzw then k_gif_rgb (sdsj_gif.hip)
hipError_t launch_gif(int n, ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, const int32_t* lengths,
                      uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s, uint64_t rm = kAllRoutes,
                      uint64_t hint = kAllRoutes);
// WebP samples (route kRtWebp; engines with SDSJ_FORMAT_WEBP): k_webp_decode, k_webp_inverse, k_webp_rgb (sdsj_webp.hip)
hipError_t launch_webp(int n, ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, const int32_t* lengths,
                       uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s, uint64_t rm = kAllRoutes,
                       uint64_t hint = kAllRoutes);
// TIFF samples (route kRtTiff; engines with SDSJ_FORMAT_TIFF): k_tiff_copy, k_tiff_lzw, k_tiff_inflate, k_tiff_rgb (sdsj_tiff.hip)
hipError_t launch_tiff(int n, ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, const int32_t* lengths,
                       uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s, uint64_t rm = kAllRoutes,
                       uint64_t hint = kAllRoutes);
// launch_png's kernels of the wider subset (sdsj_png_ext.hip); g: launch_png's grid
void launch_png_inflate_ext(unsigned g, ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, const int32_t* lengths,
                            uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s);
void launch_png_unfilter_ext(unsigned g, const ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, uint8_t* scratch,
                             const int32_t* routes, int cap, hipStream_t s);
// SDSJ_FORMAT_PNG_META (sdsj_png_meta.hip).  launch_png_meta: k_png_meta between k_parse and k_plan -- the
// compressed chunks and the chunks after the image data of every PNG sample k_parse accepted, refused ones
// turned SDSJ_UNSUPPORTED before anything is planned for them.  launch_png_inflate_meta: launch_png's
// inflate kernel under that mask (with or without SDSJ_FORMAT_PNG_EXT), which leaves the tail to k_png_meta.
hipError_t launch_png_meta(int n, ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, const int32_t* lengths,
                           hipStream_t s, int formats);
void launch_png_inflate_meta(unsigned g, ImgDesc* descs, const uint8_t* blob, const int64_t* offsets, const int32_t* lengths,
                             uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s);
// The host's side of k_png_meta (host planning, the probe): png_meta_check on one sample png_parse accepted.
int host_png_meta(const uint8_t* png, int64_t n, int64_t idat_pos, int formats);
// base: scratch bytes a previous lane of the batch already took (device), or null
hipError_t launch_plan(int n, ImgDesc* descs, int64_t capacity, const int64_t* base, int64_t* total, int32_t* routes,
                       int cap, hipStream_t s);
hipError_t launch_unstuff(int n, const uint8_t* blob, const int64_t* offsets, ImgDesc* descs, uint8_t* scratch,
                          const int32_t* routes, int cap,
                          hipStream_t s, uint64_t rm = kAllRoutes, uint64_t hint = kAllRoutes);
hipError_t launch_scanmap(int n, const uint8_t* blob, const int64_t* offsets, ImgDesc* descs, uint8_t* scratch,
                          hipStream_t s);
// progressive images (route kRtProg): zero their coefficients, then one lane per image decodes all scans
hipError_t launch_prog(int n, ImgDesc* descs, ImgTables* tables, const uint8_t* blob, const int64_t* offsets,
                       const int32_t* lengths, uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s,
                       uint64_t rm = kAllRoutes, uint64_t hint = kAllRoutes);
// progressive images of four components (route kRtProg4; engines with SDSJ_FORMAT_JPEG_CMYK_PROG): the same sequence
// through the four-component instantiations k_prog4, k_prog4_dcs and k_prog4_smooth
hipError_t launch_prog4(int n, ImgDesc* descs, ImgTables* tables, const uint8_t* blob, const int64_t* offsets,
                        const int32_t* lengths, uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s,
                        uint64_t rm = kAllRoutes, uint64_t hint = kAllRoutes);
// k_prog_zero (sdsj_progressive.hip) over the images of route rt (kRtProg, kRtProg4 or kRtScans): their int16 coefficient arrays zeroed
void launch_coef_zero(int rt, int n, const ImgDesc* descs, uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s,
                      uint64_t hint);
// multi-scan sequential images and four-component ones (route kRtScans; engines with SDSJ_FORMAT_JPEG_SCANS or
// SDSJ_FORMAT_JPEG_CMYK): zero their coefficients, then
// one wave per image decodes every scan (sdsj_scans.hip)
hipError_t launch_scans(int n, ImgDesc* descs, ImgTables* tables, const uint8_t* blob, const int64_t* offsets,
                        const int32_t* lengths, uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s,
                        uint64_t rm = kAllRoutes, uint64_t hint = kAllRoutes);
// The entry-point store for one lane of the device-resident path (sdsj_common.h HintHdr; null: off): the
// store, the lane's work lists (hint_lane_ints) and the engine's SDSJ_HINT_CTR_* counters, and the lane's
// samples, whose addresses are the keys.
struct HintLane {
  HintStore store;
  int32_t* lane;
  unsigned long long* ctr;
  const uint8_t* blob;
  const int64_t* offsets;
  const int32_t* lengths;
};
size_t enttab_bytes();  // per-image decode tables (k_enttab) held in HBM between the entropy kernels
// k_enttab (decode tables) + k_entspec (subsequence layout, warm-up, speculative decode)
// (small: a host-path latency-mode chunk, where ImgDesc::mh images take the multi-hypothesis pass)
hipError_t launch_entspec(int n, ImgDesc* descs, const ImgTables* specs, void* etab, uint8_t* scratch, int32_t* routes,
                          int cap, hipStream_t s, uint64_t rm = kAllRoutes, bool small = false,
                          uint64_t hint = kAllRoutes, const HintLane* hl = nullptr);
// k_entsync (sync rounds + segmented scan)
hipError_t launch_entsync(int n, ImgDesc* descs, void* etab, uint8_t* scratch, int32_t* routes, int cap, hipStream_t s,
                          uint64_t rm = kAllRoutes, uint64_t hint = kAllRoutes, const HintLane* hl = nullptr);
// (small: as for launch_entspec -- the lane's images are in latency mode and keep int16 coefficient blocks)
hipError_t launch_entwrite(int n, ImgDesc* descs, const void* etab, uint8_t* scratch, int32_t* routes, int cap,
                           hipStream_t s, uint64_t rm = kAllRoutes, uint64_t hint = kAllRoutes, bool small = false,
                           const HintLane* hl = nullptr);
hipError_t launch_idct(int n, const ImgDesc* descs, const ImgTables* tables, uint8_t* scratch, hipStream_t s);
// four-component images (CMYK / YCCK; engines with SDSJ_FORMAT_JPEG_CMYK), which k_idct<kMaxComp> and k_color skip:
// k_idct<4> (sdsj_idct.hip) over the lane's images, k_cmyk<RT> (sdsj_unfused.hip) over the list of route rt -- kRtScans:
// the sequential ones, kRtProg4: the progressive ones of SDSJ_FORMAT_JPEG_CMYK_PROG --; both take only the images of
// four components
hipError_t launch_idct4(int n, const ImgDesc* descs, const ImgTables* tables, uint8_t* scratch, hipStream_t s,
                        uint64_t rm = kAllRoutes);
hipError_t launch_cmyk(int rt, int n, const ImgDesc* descs, uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s,
                       uint64_t rm = kAllRoutes, uint64_t hint = kAllRoutes);
hipError_t launch_color(int n, const ImgDesc* descs, uint8_t* scratch, const int32_t* routes, int cap, hipStream_t s,
                        uint64_t rm = kAllRoutes);
hipError_t launch_coeffs(int n, ImgDesc* descs, const sdsj_op& op, uint8_t* scratch, hipStream_t s);
hipError_t launch_hpass(int n, const ImgDesc* descs, const sdsj_op& op, uint8_t* scratch, const int32_t* routes, int cap,
                        hipStream_t s, uint64_t rm = kAllRoutes);
hipError_t launch_vpass(int n, const ImgDesc* descs, const sdsj_op& op, const uint8_t* scratch, const uint8_t* flip,
                        void* out, const int32_t* routes, int cap, const float* lut, hipStream_t s,
                        uint64_t rm = kAllRoutes);
hipError_t launch_resample(int n, const ImgDesc* descs, const sdsj_op& op, const uint8_t* scratch, const uint8_t* flip,
                           void* out, int32_t* status, const int32_t* routes, int cap, const float* lut, hipStream_t s,
                           uint64_t rm = kAllRoutes, uint64_t hint = kAllRoutes);
hipError_t launch_resample420(int n, const ImgDesc* descs, const sdsj_op& op, int strip_h, const uint8_t* scratch,
                              const uint8_t* flip, void* out, const int32_t* routes, int cap, const float* lut,
                              hipStream_t s, uint64_t rm = kAllRoutes, uint64_t hint = kAllRoutes);
// lengths: the samples' encoded sizes (null: raw frames); counters: SDSJ_CTR_* accumulators (or null)
// (a negative length: the sample is reported as EINVAL -- an unreadable file of the host path)
hipError_t launch_finish(int n, ImgDesc* descs, const sdsj_op& op, void* out, int32_t* status, const float* lut,
                         const int32_t* lengths, unsigned long long* counters, hipStream_t s);
// host-side planning (plan_sample of sdsj_plan.h, as k_parse runs it, without k_parse's validation of the
// Huffman tables): returns the scratch bytes image `jpg` needs (0 unless *status is SDSJ_OK)
// *routes (optional): the routes the image takes (bits as in route masks; all of them when the host
// parse fails, so the device's own verdict is never starved of a kernel)
// small: the latency-mode plan of a chunk of at most kSmallBatch images (k_parse's `small`)
// *later (optional): the status the device reports for the sample after planning where host planning knows it
// (a multi-scan sequential file k_scans refuses, scans_check; SDSJ_OK otherwise): the sample is sized and routed
// like a good one, as the device sizes it
int64_t host_plan_need(const uint8_t* jpg, int64_t n, const sdsj_op& op, int* status, uint64_t* routes = nullptr,
                       bool small = false, int formats = SDSJ_FORMAT_JPEG, int* later = nullptr);
// host-side planning of one raw RGB frame (width x height) for the unfused passes; returns scratch bytes
int64_t host_plan_frame(ImgDesc* d, int width, int height, const sdsj_op& op);
}  // namespace sdsj
