// Host AddressSanitizer / UBSan driver of the shared PNG core under SDSJ_FORMAT_PNG_META: the functions
// k_parse and k_png_meta run for files with iCCP, zTXt and iTXt chunks and with chunks after the image data
// -- png_parse with the mask (png_chunk_ok, png_meta_stream), then png_meta_check (png_meta_chunk, the
// count-only inflate png_inflate_count, the walk over the tail).  Like tests/asan/png_ext_driver.cpp it reads
// records [u32 length][bytes] from the file in argv[1]; it prints one line per record: the status under
// mask 19 (JPEG | PNG | PNG_META) and under mask 23 (with PNG_EXT), width, height.  Each input is an exactly
// sized heap block, so a read outside [0, n) is reported.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../sds_amd/csrc/sdsj_png.h"

using namespace sdsj;

struct Rd {
  const uint8_t* p;
  int operator()(int64_t i) const { return p[i]; }
};

static int status(const uint8_t* buf, int64_t n, int formats, PngHdr* h, InfTables* T) {
  Rd rd{buf};
  int st = png_parse(rd, n, h, formats);
  if (st == SDSJ_OK) st = png_meta_check(rd, n, h->idat_pos, formats, T);
  return st;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> all;
  static uint8_t tmp[1 << 16];
  size_t r;
  while ((r = fread(tmp, 1, sizeof(tmp), f)) > 0) all.insert(all.end(), tmp, tmp + r);
  fclose(f);
  InfTables* T = new InfTables();
  size_t pos = 0;
  while (pos + 4 <= all.size()) {
    uint32_t n;
    memcpy(&n, &all[pos], 4);
    pos += 4;
    if (pos + n > all.size()) return 3;
    uint8_t* buf = static_cast<uint8_t*>(malloc(n ? n : 1));
    memcpy(buf, &all[pos], n);
    pos += n;
    PngHdr h;
    const int meta = SDSJ_FORMAT_JPEG | SDSJ_FORMAT_PNG | SDSJ_FORMAT_PNG_META;
    const int st19 = status(buf, (int64_t)n, meta, &h, T);
    const int st23 = status(buf, (int64_t)n, meta | SDSJ_FORMAT_PNG_EXT, &h, T);
    printf("%d %d %d %d\n", st19, st23, h.width, h.height);
    free(buf);
  }
  delete T;
  return 0;
}
