// Host AddressSanitizer / UBSan driver of the planner (sds_amd/csrc/sdsj_plan.h): plan_sample, the code
// k_parse lane 0 and host planning run, then image_routes.  Reads records
//   [i32 out_h][i32 out_w][i32 crop_before_resize][i32 filter][i32 small][i32 formats][u32 length][bytes]
// from the file in argv[1].  The first output line holds kRtUnfused and kRtPng; then one line per record:
//   status, the 14 plan fields (geo cx0 cy0 cw ch need_h need_v ksh ksv ring_rows fused tile_w rs_fast
//   rs_lay), the routes (unstuff entropy resample; -9 each unless the status is OK), need (0 unless OK), the
//   13 off_* fields in plan_image's order, width height ncomp, then the entropy / unstuff plan: entropy_len nseg
//   ntiles sub_bits nsub_cap warm_bits ent_groups lat mh, and warm_small: the warm_bits k_parse gives the image
//   in a lane of fewer than kWarmSmallLane images (plan_image itself plans for a large lane).
// `plan_driver --constants` prints instead "name value" lines: the routes, the thresholds the entropy case table
// reads (tests/entropy_cases.py) and SubState's layout (tests/gpu_debug.py), as the compiler sees them.
// Each sample is copied into an exactly sized heap buffer, so any read past its end is reported.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <stddef.h>

#include <vector>

#include "../../sds_amd/csrc/sdsj_plan.h"

using namespace sdsj;

#define SDSJ_PRINT(x) printf(#x " %lld\n", (long long)(x))

static int print_constants() {
  SDSJ_PRINT(kRtEnt10);
  SDSJ_PRINT(kRtEnt11);
  SDSJ_PRINT(kRtEnt11M);
  SDSJ_PRINT(kRtProg);
  SDSJ_PRINT(kRtUsSmall);
  SDSJ_PRINT(kRtUsBig);
  SDSJ_PRINT(kRtScans);
  SDSJ_PRINT(kDecodeThreads);
  SDSJ_PRINT(kMinSubBits);
  SDSJ_PRINT(kWarmBits);
  SDSJ_PRINT(kWarmBitsSmall);
  SDSJ_PRINT(kWarmSmallLane);
  SDSJ_PRINT(kWarmDiv);
  SDSJ_PRINT(kSmallBatch);
  SDSJ_PRINT(kLatSubBits);
  SDSJ_PRINT(kLatWarm);
  SDSJ_PRINT(kGroupBits);
  SDSJ_PRINT(kMaxEntGroups);
  SDSJ_PRINT(kUsTileBytes);
  SDSJ_PRINT(kUsSerialTiles);
  SDSJ_PRINT(kRec);
  SDSJ_PRINT(sizeof(SubState));
  SDSJ_PRINT(offsetof(SubState, start_bit));
  SDSJ_PRINT(offsetof(SubState, end_bit));
  SDSJ_PRINT(offsetof(SubState, first));
  SDSJ_PRINT(offsetof(SubState, seg));
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "--constants")) return print_constants();
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> all;
  uint8_t tmp[1 << 16];
  size_t r;
  while ((r = fread(tmp, 1, sizeof(tmp), f)) > 0) all.insert(all.end(), tmp, tmp + r);
  fclose(f);
  printf("%d %d\n", (int)kRtUnfused, (int)kRtPng);
  size_t pos = 0;
  while (pos + 28 <= all.size()) {
    int32_t h[6];
    uint32_t n;
    memcpy(h, &all[pos], 24);
    memcpy(&n, &all[pos + 24], 4);
    pos += 28;
    if (pos + n > all.size()) return 3;
    uint8_t* buf = static_cast<uint8_t*>(malloc(n ? n : 1));
    memcpy(buf, &all[pos], n);
    pos += n;
    sdsj_op op{};
    op.out_h = h[0];
    op.out_w = h[1];
    op.crop_before_resize = h[2];
    op.filter = h[3];
    ImgDesc* d = new ImgDesc();
    ImgTables* t = new ImgTables();
    MemReader rd{buf};
    const int st = plan_sample(rd, (int64_t)n, op, h[4] != 0, h[5], d, t, CopySink<MemReader>{rd});
    int ru = -9, re = -9, rr = -9;
    if (st == SDSJ_OK) image_routes(*d, &ru, &re, &rr);
    printf("%d  %d %d %d %d %d %d %d %d %d %d %d %d %d %d  %d %d %d  %lld ", st, d->geo, d->cx0, d->cy0, d->cw, d->ch,
           d->need_h, d->need_v, d->ksh, d->ksv, d->ring_rows, d->fused, d->tile_w, d->rs_fast, d->rs_lay, ru, re, rr,
           st == SDSJ_OK ? (long long)d->need : 0LL);
    const int64_t offs[13] = {d->off_ustream, d->off_seg, d->off_tiles,  d->off_sub, d->off_rec, d->off_ptab, d->off_coef,
                              d->off_planes,  d->off_rgb, d->off_tmp,    d->off_kh,  d->off_kv,  d->off_png};
    for (int k = 0; k < 13; k++) printf(" %lld", (long long)offs[k]);
    printf("  %d %d %d", d->width, d->height, d->ncomp);
    printf("  %lld %d %d %d %d %d %d %d %d %d\n", (long long)d->entropy_len, d->nseg, d->ntiles, d->sub_bits, d->nsub_cap,
           d->warm_bits, d->ent_groups, d->lat, (int)d->mh, d->lat ? d->warm_bits : warm_for(d->sub_bits, kWarmBitsSmall));
    delete d;
    delete t;
    free(buf);
  }
  return pos == all.size() ? 0 : 3;
}
