// Host AddressSanitizer / UBSan driver of the parser and planner under the "jpeg-cmyk-prog" masks
// (sds_amd/csrc/sdsj_plan.h): plan_sample with SDSJ_FORMAT_JPEG | SDSJ_FORMAT_JPEG_CMYK | SDSJ_FORMAT_JPEG_CMYK_PROG alone
// (1537), with SDSJ_FORMAT_JPEG_EXT (1601), with SDSJ_FORMAT_JPEG_SCANS (1665) and with both (1729) -- the code k_parse
// lane 0 and host planning run, the fourth component's packed record and the larger table state of a progressive
// four-component image included --, then, as host planning does, scans_check and image_routes.  Reads [u32 length][bytes] records from the file in argv[1]; every sample is planned for a 16 x 20
// bilinear resize without the centre crop.  One output line per record, four integers per mask in the order above:
//   status, need, the progressive field, the entropy route (0, 0, -9 unless the plan is OK: a file scans_check
//   refuses keeps the plan's)
// and then kRtProg4, kRtScans and the component count the last mask parsed.
// Each sample is copied into an exactly sized heap buffer, so any read past its end is reported.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../sds_amd/csrc/sdsj_plan.h"

using namespace sdsj;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> all;
  uint8_t tmp[1 << 16];
  size_t r;
  while ((r = fread(tmp, 1, sizeof(tmp), f)) > 0) all.insert(all.end(), tmp, tmp + r);
  fclose(f);
  const int base = SDSJ_FORMAT_JPEG | SDSJ_FORMAT_JPEG_CMYK | SDSJ_FORMAT_JPEG_CMYK_PROG;
  const int masks[4] = {base, base | SDSJ_FORMAT_JPEG_EXT, base | SDSJ_FORMAT_JPEG_SCANS,
                        base | SDSJ_FORMAT_JPEG_EXT | SDSJ_FORMAT_JPEG_SCANS};
  size_t pos = 0;
  while (pos + 4 <= all.size()) {
    uint32_t n;
    memcpy(&n, &all[pos], 4);
    pos += 4;
    if (pos + n > all.size()) return 3;
    uint8_t* buf = static_cast<uint8_t*>(malloc(n ? n : 1));
    memcpy(buf, &all[pos], n);
    pos += n;
    sdsj_op op{};
    op.out_h = 16;
    op.out_w = 20;
    op.crop_before_resize = 0;
    op.filter = SDSJ_FILTER_BILINEAR;
    int ncomp = 0;
    for (int k = 0; k < 4; k++) {
      ImgDesc* d = new ImgDesc();
      ImgTables* t = new ImgTables();
      MemReader rd{buf};
      int st = plan_sample(rd, (int64_t)n, op, false, masks[k], d, t, CopySink<MemReader>{rd});
      const bool ok = st == SDSJ_OK;
      if (ok && d->progressive == kScansSequential) st = scans_check(rd, (int64_t)n, *d);
      int ru = -9, re = -9, rr = -9;
      if (ok) image_routes(*d, &ru, &re, &rr);
      printf("%d %lld %d %d ", st, ok ? (long long)d->need : 0LL, ok ? d->progressive : 0, re);
      ncomp = d->ncomp;
      delete d;
      delete t;
    }
    printf("%d %d %d\n", (int)kRtProg4, (int)kRtScans, ncomp);
    free(buf);
  }
  return pos == all.size() ? 0 : 3;
}
