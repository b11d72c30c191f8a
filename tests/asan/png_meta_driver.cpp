// Host AddressSanitizer / UBSan driver of the shared PNG core under SDSJ_FORMAT_PNG_META: the functions
// k_parse and k_png_meta run for files with iCCP, zTXt and iTXt chunks and with chunks after the image data
// -- png_parse with the mask (png_chunk_ok, png_meta_stream), then png_meta_check (png_meta_chunk, the
// count-only inflate png_inflate_count, the walk over the tail).  Like tests/asan/png_ext_driver.cpp it reads
// records [u32 length][bytes] from the file in argv[1]; it prints one line per record: the status under
// mask 19 (JPEG | PNG | PNG_META) and under mask 23 (with PNG_EXT), width, height.  Each input is an exactly
// sized heap block, so a read outside [0, n) is reported.
#include "png_driver_common.h"

static int status(const uint8_t* buf, int64_t n, int formats, PngHdr* h, InfTables* T) {
  Rd rd{buf};
  int st = png_parse(rd, n, h, formats);
  if (st == SDSJ_OK) st = png_meta_check(rd, n, h->idat_pos, formats, T);
  return st;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  InfTables* T = new InfTables();
  const int rc = for_each_record(argv[1], [T](const uint8_t* buf, int64_t n) {
    PngHdr h;
    const int meta = SDSJ_FORMAT_JPEG | SDSJ_FORMAT_PNG | SDSJ_FORMAT_PNG_META;
    const int st19 = status(buf, n, meta, &h, T);
    const int st23 = status(buf, n, meta | SDSJ_FORMAT_PNG_EXT, &h, T);
    printf("%d %d %d %d\n", st19, st23, h.width, h.height);
  });
  delete T;
  return rc;
}
