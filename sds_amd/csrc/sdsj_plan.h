// sdsj_plan.h -- the planner, shared by host and device: what decides every scratch offset the later
// kernels trust (plan_image: off_ustream .. off_png, need) and the kernel an image gets (image_routes),
// and the one sequence that leads there -- choose the format, parse the headers, set up the geometry,
// plan (plan_sample).  k_parse runs it on the device, host planning (host_plan_need), sdsj_probe and the
// sanitized drivers under tests/asan on the host: one implementation, compiled for both sides.
#pragma once
#include <stdint.h>

#include "sdsj_common.h"
#include "sdsj_gif.h"
#include "sdsj_png.h"
#include "sdsj_tiff.h"
#include "sdsj_webp.h"

namespace sdsj {

// The host byte reader: byte i of a sample in memory.
struct MemReader {
  const uint8_t* p;
  int operator()(int64_t i) const { return p[i]; }
};

// Pillow precompute_coeffs bounds for output index xx (doubles, same operation order).
SDSJ_HD inline void resample_bounds(int in_size, int out_size, double support_base, int xx,
                                    int* xmin_out, int* xmax_out) {
  double scale = (double)in_size / out_size;
  double filterscale = scale < 1.0 ? 1.0 : scale;
  double support = support_base * filterscale;
  double center = 0.0 + (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  *xmin_out = xmin;
  *xmax_out = xmax - xmin;
}

// Speculative warm-up of a subsequence of sub_bits: floor_bits, or sub_bits / kWarmDiv when that is
// larger, and at most 1.5 x sub_bits.
SDSJ_HD inline int warm_for(int sub_bits, int floor_bits) {
  const int w = sub_bits / kWarmDiv > floor_bits ? sub_bits / kWarmDiv : floor_bits;
  return sub_bits * 3 / 2 < w ? sub_bits * 3 / 2 : w;
}

// frames = true: raw RGB frames (sdsj_resize_frames_device): the unfused passes read the frame rows
// in place (off_rgb / rgb_pitch are set by the caller), no entropy / plane / RGB-row scratch.
// png = true: a PNG sample: like a frame it resamples through the unfused passes, from RGB rows that
// k_png_unfilter packs at off_rgb; its inflated scanlines take off_png.
SDSJ_HD inline int64_t plan_image(ImgDesc* d, const sdsj_op& op, bool frames = false, bool small = false,
                                  bool png = false) {
  // Geometry: functional.py:78-80 shortcut, :118-147 crop, Pillow ImagingResampleInner.
  const int W = d->width, H = d->height;
  if (W == op.out_w && H == op.out_h) {
    d->geo = kGeoIdentity;
    d->cx0 = d->cy0 = 0;
    d->cw = W;
    d->ch = H;
  } else {
    d->geo = kGeoResize;
    if (op.crop_before_resize) {
      crop_box(W, H, op.out_h, op.out_w, &d->cx0, &d->cy0, &d->cw, &d->ch);
    } else {
      d->cx0 = d->cy0 = 0;
      d->cw = W;
      d->ch = H;
    }
    if (d->cw <= 0 || d->ch <= 0) d->geo = kGeoZeros;
  }
  d->need_h = d->geo == kGeoResize && d->cw != op.out_w;
  d->need_v = d->geo == kGeoResize && d->ch != op.out_h;
  // NEAREST (Pillow ImagingScaleAffine) runs as a one-tap resample through the unfused passes: tap
  // weight 1 << 22 at the source index nearest_src picks, none where it is outside (fill value 0)
  const bool nearest = op.filter == SDSJ_FILTER_NEAREST;
  double sup = filter_support(op.filter);
  d->ksh = d->need_h ? (nearest ? 1 : resample_ksize(d->cw, op.out_w, sup)) : 0;
  d->ksv = d->need_v ? (nearest ? 1 : resample_ksize(d->ch, op.out_h, sup)) : 0;
  if (d->geo == kGeoZeros) {
    d->yf = d->yl = 0;
  } else if (d->need_v && nearest) {
    const int a = nearest_src(d->ch, op.out_h, 0), b = nearest_src(d->ch, op.out_h, op.out_h - 1);
    d->yf = a < 0 || b < 0 ? 0 : a;
    d->yl = a < 0 || b < 0 ? d->ch : b + 1;
  } else if (d->need_v) {
    int a0, a1, b0, b1;
    resample_bounds(d->ch, op.out_h, sup, 0, &a0, &a1);
    resample_bounds(d->ch, op.out_h, sup, op.out_h - 1, &b0, &b1);
    d->yf = a0;
    d->yl = b0 + b1;
  } else {
    d->yf = 0;
    d->yl = d->ch;
  }
  d->src_y0 = d->cy0 + d->yf;
  d->src_y1 = d->cy0 + d->yl;
  d->src_x0 = d->cx0;
  d->src_w = d->geo == kGeoZeros ? 0 : d->cw;
  // fused resample tiles: halve the tile width until a tile's source columns fit kMaxSpan
  // (bound: (tw - 1) * scale + 2 * support + 2 columns, Pillow precompute_coeffs windows)
  d->fused = 0;
  d->tile_w = 0;
  double span = 0.0;  // the tile's source-column bound
  d->ring_rows = 1;
  while (d->ring_rows < d->ksv) d->ring_rows *= 2;  // vertical window rows kept per column
  if (d->geo != kGeoZeros && d->ring_rows <= kRingMaxRows && !nearest) {
    const double scale = d->need_h ? (double)d->cw / op.out_w : 1.0;
    const double supp = d->need_h ? sup * (scale < 1.0 ? 1.0 : scale) : 0.0;
    int tw = op.out_w < 256 ? op.out_w : 256;
    if (tw > kRingDW / d->ring_rows) tw = kRingDW / d->ring_rows;
    const int lim = d->ksh <= 7 ? rs_span(d->ksh) : kMaxSpan;  // (the KT <= 7 fused kernels' rows)
    for (;;) {
      span = (double)tw * scale + 2.0 * supp + 4.0;
      if (span <= (double)lim) {
        d->fused = 1;
        d->tile_w = tw;
        break;
      }
      if (tw == 1) break;
      tw = (tw + 1) / 2;
    }
  }
  if (frames || png) d->fused = 0;
  // SDSJ_FORMAT_JPEG_EXT images (RGB-coded, or a ratio above 2): the unfused passes, whose k_color
  // restates every upsampling method and the missing colour transform
  else if (jpeg_ext_image(*d)) d->fused = 0;
  // SDSJ_FORMAT_JPEG_CMYK images (four components): the unfused passes too, behind a colour kernel of their
  // own (k_cmyk), which writes the RGB rows k_color writes for the others
  else if (d->ncomp > kMaxComp) d->fused = 0;
  // specialised fused kernels (sdsj_resample420.hip): 4:2:0 (h2v2 fancy chroma), 4:2:2 (h2v1 fancy
  // chroma), 4:4:4 and grayscale, horizontal and vertical passes, odd tap counts 3..11; everything
  // else takes the generic k_resample
  d->rs_fast = 0;
  d->rs_lay = kRs420;
  if (d->fused && d->need_h && d->need_v && d->ksh >= 3 && d->ksh <= 11 && (d->ksh & 1) &&
      d->ring_rows <= rs_ring_rows(d->ksh) && d->ksv <= rs_vtaps(d->ksh) && d->tile_w * d->ring_rows <= rs_ring_dw(d->ksh) &&
      span <= (double)rs_span(d->ksh) && d->comp[0].rh == 1 && d->comp[0].rv == 1) {
    const CompDesc &c1 = d->comp[1], &c2 = d->comp[2];
    const bool same = d->ncomp == 3 && c2.rh == c1.rh && c2.rv == c1.rv && c2.dw == c1.dw && c2.dh == c1.dh;
    int lay = -1;
    if (d->ncomp == 1) lay = kRsGray;
    else if (same && c1.rh == 1 && c1.rv == 1) lay = kRs444;
    else if (same && c1.rh == 2 && c1.rv == 1 && c1.dw > 2) lay = kRs422;
    else if (same && c1.rh == 2 && c1.rv == 2 && c1.dw > 2) lay = kRs420;
    if (lay >= 0) {
      d->rs_fast = d->ksh;
      d->rs_lay = lay;
    }
  }
  d->lat = small && !frames && !png;
  // multi-hypothesis speculative pass for latency-mode baseline images without restart intervals;
  // only the 11-bit entropy routes launch it (k_entspec_mh), so images of more than 4 table slots
  // (kRtEnt10) keep the ordinary speculative pass
  // (the table slots, counted once: they also choose the coefficient format; frames and PNGs have no scan)
  // (a four-component image is walked by k_scans, which counts no slots: int16 blocks whatever they are)
  const int slots = frames || png || d->ncomp > kMaxComp ? 2 * kMaxComp : huff_slots(*d);
  d->mh = (int8_t)(SDSJ_MH && d->lat && !d->progressive && d->restart_interval == 0 && d->bpm <= kMhMaxPhases &&
                   slots <= 4);
  d->hinted = 0;  // (k_enthint sets it)
  {
    const int64_t bits = d->entropy_len * 8;
    const int64_t per_group = (int64_t)kDecodeThreads * (d->lat ? kLatSubBits : kGroupBits);
    int64_t g = (bits + per_group - 1) / per_group;
    g = g < 1 ? 1 : (g > kMaxEntGroups ? kMaxEntGroups : g);
    d->ent_groups = frames || png ? 1 : (int32_t)g;
    const int64_t lanes = (int64_t)kDecodeThreads * d->ent_groups;
    d->sub_bits = (int32_t)align_up((bits + lanes - 1) / lanes, 32);
  }
  const int min_sub = d->lat ? kLatSubBits : kMinSubBits;
  if (d->sub_bits < min_sub) d->sub_bits = min_sub;
  // warm-up: kWarmBits (k_parse may raise the floor for small lanes), or sub_bits / kWarmDiv for long
  // subsequences (large images: a few percent more speculative work removes nearly every sync task,
  // each of which is a serial re-decode); latency mode: kLatWarm
  d->warm_bits = d->lat ? kLatWarm : warm_for(d->sub_bits, kWarmBits);
  d->nsub_cap = (int32_t)((d->entropy_len * 8 + d->sub_bits - 1) / d->sub_bits) + d->nseg + 1;
  const bool prog = d->progressive && !frames;  // k_prog decodes it: no unstuffed stream, no subsequences
  if (prog) {
    d->ent_groups = 1;
    d->nsub_cap = 1;
  }
  // scratch layout (relative offsets; k_plan adds the image base)
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    int64_t r = o;
    o += align_up(bytes, 256);
    return r;
  };
  d->off_ustream = take(prog ? 32 : d->entropy_len + kUPad + 32);  // + the 16-byte granule of the final pad store
  d->ustream_cap = prog ? 0 : d->entropy_len + kUPad;
  d->off_seg = take(seg_bytes(d->nseg));
  d->ntiles = prog ? 0 : (int32_t)((d->entropy_len + kUsTileBytes - 1) / kUsTileBytes);
  d->off_tiles = take((int64_t)d->ntiles * sizeof(UsTile));
  d->off_sub = take((int64_t)d->nsub_cap * sizeof(SubState));
  d->off_rec = take((int64_t)d->nsub_cap * kRec * sizeof(SyncRec));
  // (a progressive image of four components: the fourth one's latch flag and smoothing bits follow the tables)
  d->off_ptab = take(prog ? (int64_t)(prog4_image(*d) ? sizeof(ProgTables4) : sizeof(ProgTables)) : 0);
  d->off_coef = take(coef_bytes(*d, slots));
  int64_t planes = 0;
  for (int c = 0; c < d->ncomp; c++) {
    const CompDesc cd = comp_of(*d, c);
    planes += align_up((int64_t)cd.pitch * cd.bh * 8, 256);
  }
  d->off_planes = take(planes);
  d->off_rgb = take(d->fused || frames ? 0 : (int64_t)d->src_w * (d->src_y1 - d->src_y0) * 3);
  d->rgb_pitch = d->src_w;  // k_color packs the crop rows
  d->off_tmp = take(!d->fused && d->need_h ? (int64_t)(d->yl - d->yf) * op.out_w * 3 : 0);
  d->off_kh = take(d->need_h ? ((int64_t)2 * op.out_w + (int64_t)op.out_w * d->ksh) * 4 : 0);
  d->off_kv = take(d->need_v ? ((int64_t)2 * op.out_h + (int64_t)op.out_h * d->ksv) * 4 : 0);
  d->off_png = take(png ? d->png_raw + 64 : 0);
  d->need = o;
  return o;
}

// The routes of one planned image (k_plan's lists; host planning's route masks): unstuffing (-1 for
// progressive images), entropy variant by the Huffman tables in use (slots as load_tables counts
// them), resample variant as plan_image chose it (-1 for an empty crop).
SDSJ_HD inline void image_routes(const ImgDesc& d, int* ru, int* re, int* rr) {
  if (d.png) {  // (a PNG, a GIF: kGifSample, a WebP: kWebpSample, or a TIFF: kTiffSample)
    *ru = -1;
    *re = d.png == kGifSample ? kRtGif : d.png == kWebpSample ? kRtWebp : d.png == kTiffSample ? kRtTiff : kRtPng;
    *rr = d.geo == kGeoZeros ? -1 : kRtUnfused;
    return;
  }
  const int ns = d.progressive ? 0 : huff_slots(d);  // (it chooses among the baseline entropy routes only)
  *ru = d.progressive ? -1 : (d.ntiles > kUsSerialTiles || d.lat ? kRtUsBig : kRtUsSmall);
  *re = d.progressive == kScansSequential ? kRtScans : d.progressive ? (prog4_image(d) ? kRtProg4 : kRtProg) : ns > 4 ? kRtEnt10 : (d.ent_groups > 1 ? kRtEnt11M : kRtEnt11);
  *rr = d.geo == kGeoZeros ? -1
        : !d.fused ? kRtUnfused
                   : (d.rs_fast ? rs_route(d.rs_lay, d.rs_fast) : gen_route(d.need_h ? d.ksh : 1));
}

// JPEG headers up to the first SOS, then colour space and geometry.
template <class Reader, class Sink>
SDSJ_HD int parse_sample(const Reader& rd, int64_t n, ImgDesc* d, ImgTables* t, const Sink& sink,
                         int formats = SDSJ_FORMAT_JPEG) {
  int st = parse_headers(rd, n, d, t, sink, formats);
  if (st == SDSJ_OK) st = setup_geometry(d, t, formats);
  return st;
}

// The host's side of what k_scans refuses while it walks the scans of a multi-scan sequential file
// (ImgDesc::progressive == kScansSequential; every four-component file is one): a scan that is not a full sequential one or codes a
// component again (SDSJ_UNSUPPORTED: libjpeg only warns and overlays the coefficients), a malformed SOS
// and, in a scan without restart intervals, fill bytes before a stuffed zero (SDSJ_CORRUPT: k_scans'
// fill_stuffed).  A marker walk, no entropy decoding: host planning and the probe run it, so that such a file is
// not sized as a decodable one; everything else about the stream is the device's verdict.
template <class Reader>
inline int scans_check(const Reader& rd, int64_t n, const ImgDesc& d) {
  int64_t pos = d.sos_pos;
  int restart_interval = d.restart_interval, coded = 0;
  for (;;) {
    if (pos + 2 > n) return SDSJ_CORRUPT;
    const int len = (rd(pos) << 8) | rd(pos + 1);
    if (len < 3 || pos + len > n) return SDSJ_CORRUPT;
    const int ns = rd(pos + 2);
    if (ns < 1 || ns > 4 || len != 2 * ns + 6) return SDSJ_CORRUPT;  // get_sos: JERR_BAD_LENGTH
    for (int q = 0; q < ns; q++) {
      const int cid = rd(pos + 3 + 2 * q);
      int c = 0;
      while (c < d.ncomp && comp_id_of(d, c) != cid) c++;
      if (c == d.ncomp) return SDSJ_CORRUPT;
      if ((coded >> c) & 1) return SDSJ_UNSUPPORTED;
      coded |= 1 << c;
    }
    if (rd(pos + 3 + 2 * ns) != 0 || rd(pos + 4 + 2 * ns) != 63 || rd(pos + 5 + 2 * ns) != 0) return SDSJ_UNSUPPORTED;
    // the scan's data, then the segments up to the next SOS
    int64_t i = pos + len;
    bool in_scan = true;
    for (;;) {
      while (i < n && rd(i) != 0xFF) i++;
      int64_t j = i;
      while (j < n && rd(j) == 0xFF) j++;
      if (j >= n) return SDSJ_OK;  // (the input ends: the device reports it)
      const int m = rd(j);
      if (m == 0) {  // a stuffed zero
        if (in_scan && j - i >= 2 && restart_interval == 0) return SDSJ_CORRUPT;
        i = j + 1;
        continue;
      }
      if ((m >= 0xD0 && m <= 0xD7) || m == 0x01) {
        i = j + 1;
        continue;
      }
      const bool seg = (m >= 0xE0 && m <= 0xEF) || m == 0xFE || m == 0xDD || m == 0xC4 || m == 0xDB || m == 0xDA;
      if (!seg) return SDSJ_OK;  // EOI; anything else is the device's to refuse
      in_scan = false;
      if (j + 3 > n) return SDSJ_OK;
      const int l2 = (rd(j + 1) << 8) | rd(j + 2);
      if (l2 < 2 || j + 1 + l2 > n) return SDSJ_OK;
      if (m == 0xDA) {
        pos = j + 1;
        break;
      }
      if (m == 0xDD && l2 == 4) restart_interval = (rd(j + 3) << 8) | rd(j + 4);
      i = j + 1 + l2;
    }
  }
}

// Validation of the Huffman tables a baseline scan uses (huff_table_ok; a progressive image's are
// checked per scan by k_prog).  The table bytes must have been copied (CopySink).
SDSJ_HD inline bool scan_tables_ok(const ImgDesc& d, const ImgTables& t) {
  for (int c = 0; !d.progressive && c < d.ncomp; c++)
    if (!huff_table_ok(t.dc_spec[d.comp[c].td], true) || !huff_table_ok(t.ac_spec[d.comp[c].ta], false)) return false;
  return true;
}

// One sample, from its bytes to its plan: a PNG, a GIF, a WebP or a TIFF (where the engine's formats enable it) is parsed and
// planned for the unfused passes, everything else is a JPEG or SDSJ_UNSUPPORTED.  Returns the status;
// *d is planned (d->need, the off_* fields, what image_routes reads) only when it is SDSJ_OK.  Table
// validation is not part of it: the device's sink defers the table bytes (k_parse validates once all
// lanes have copied them), and host planning never validated them.
template <class Reader, class Sink>
SDSJ_HD int plan_sample(const Reader& rd, int64_t n, const sdsj_op& op, bool small, int formats, ImgDesc* d,
                        ImgTables* t, const Sink& sink) {
  int status;
  d->png = 0;
  if ((formats & SDSJ_FORMAT_PNG) && png_signature(rd, n)) {
    PngHdr ph;
    status = png_parse(rd, n, &ph, formats);
    png_fill_desc(d, ph);
    if (status == SDSJ_OK) plan_image(d, op, false, false, true);
  } else if ((formats & SDSJ_FORMAT_GIF) && gif_signature(rd, n)) {
    // (planned like a PNG: the index buffer takes off_png -- png_raw = width x height bytes --, k_gif_rgb
    // packs the RGB rows at off_rgb)
    GifHdr gh;
    status = gif_parse(rd, n, &gh);
    gif_fill_desc(d, gh);
    if (status == SDSJ_OK) plan_image(d, op, false, false, true);
  } else if ((formats & SDSJ_FORMAT_WEBP) && webp_signature(rd, n)) {
    // (planned like a PNG: off_png takes webp_layout's bytes -- png_raw, an upper bound known from width and
    // height --, k_webp_rgb packs the RGB rows at off_rgb)
    WebpHdr wh;
    status = webp_parse(rd, n, &wh);
    webp_fill_desc(d, wh);
    if (status == SDSJ_OK) plan_image(d, op, false, false, true);
  } else if ((formats & SDSJ_FORMAT_TIFF) && tiff_signature(rd, n)) {
    // (planned like a PNG: off_png takes the decoded strips -- png_raw = height x width x samples bytes --,
    // k_tiff_rgb packs the RGB rows at off_rgb)
    TiffHdr th;
    status = tiff_parse(rd, n, &th);
    tiff_fill_desc(d, th);
    if (status == SDSJ_OK) plan_image(d, op, false, false, true);
  } else if (!(formats & SDSJ_FORMAT_JPEG)) {
    status = SDSJ_UNSUPPORTED;
  } else {
    status = parse_sample(rd, n, d, t, sink, formats);
    if (status == SDSJ_OK) plan_image(d, op, false, small);
  }
  return status;
}

}  // namespace sdsj
