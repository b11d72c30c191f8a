/*
 * sdsj.h -- C-ABI of the MI355X-native JPEG decode + crop/resize/flip/normalise path.
 *
 * The reference (snap-research/sds) has no native boundary: its image hot path is the Python
 * transform list built by create_standard_image_pipeline (sds/transforms/presets.py:716-744),
 * whose arithmetic runs in Pillow/libjpeg-turbo.  Each entry point below replaces one piece of
 * that list; the Python drop-in (sds_amd/presets.py) binds them with ctypes, exactly as a
 * maintainer would add a ctypes stub to sds (INTEGRATION.md shows that binding):
 *
 *   sdsj_probe                      <- PIL.Image.open() header parse inside
 *                                      load_image_from_bytes (functional.py:94-100)
 *   sdsj_decode_resize_batch        <- DecodeImageTransform (presets.py:39-45) +
 *                                      ResizeImageTransform (presets.py:47-58 -> functional.py:38-86,
 *                                      crop functional.py:118-147) +
 *                                      ConvertImageToByteTensorTransform (presets.py:68-74 ->
 *                                      functional.py:102-110) + optional
 *                                      NormalizeFramesTransform (presets.py:154-162) and the
 *                                      user hflip (README.md:99-108), inputs in host memory
 *   sdsj_decode_resize_batch_device <- the same, inputs already resident in device memory
 *                                      (the device-resident benchmark, configs 2-4)
 *   sdsj_engine_create/destroy      <- (no reference counterpart: per-process GPU state that the
 *                                      transform creates lazily, presets.py:1-5 pickling rule)
 *
 * Conventions: plain C types only; every function returns an int status (0 = SDSJ_OK, < 0 an
 * error) and never throws; pointers are borrowed for the duration of the call.  All device work
 * is enqueued on the caller's HIP stream (hipStream_t passed as void*).
 */
#ifndef SDSJ_H
#define SDSJ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDSJ_ABI_VERSION 2 /* 2: blob_bytes on the device entry point */

/* status codes (per call and per sample) */
#define SDSJ_OK 0
#define SDSJ_EINVAL (-1)      /* bad argument */
#define SDSJ_UNSUPPORTED (-2) /* valid JPEG the MI355X path does not decode (arithmetic, 12-bit, CMYK without SDSJ_FORMAT_JPEG_CMYK, ...) */
#define SDSJ_CORRUPT (-3)     /* malformed / truncated stream (PIL raises OSError) */
#define SDSJ_ENOMEM (-4)      /* allocation failed */
#define SDSJ_EHIP (-5)        /* HIP runtime error (see sdsj_last_error) */
#define SDSJ_ECAPACITY (-6)   /* sample did not fit the engine's scratch; resubmit in a smaller batch */

/* resampling filters (Pillow Image.Resampling numbering is not used; see sds_amd/presets.py) */
#define SDSJ_FILTER_BOX 0
#define SDSJ_FILTER_BILINEAR 1
#define SDSJ_FILTER_HAMMING 2
#define SDSJ_FILTER_BICUBIC 3
#define SDSJ_FILTER_LANCZOS 4
#define SDSJ_FILTER_NEAREST 5 /* Pillow NEAREST (ImagingScaleAffine), torchvision 'nearest' / 'nearest-exact' on PIL */

#define SDSJ_DTYPE_U8 0  /* uint8 samples, as ConvertImageToByteTensorTransform */
#define SDSJ_DTYPE_F32 1 /* float32 x/127.5-1, as NormalizeFramesTransform */

#define SDSJ_LAYOUT_CHW 0 /* [3][H][W] contiguous */
#define SDSJ_LAYOUT_HWC 1 /* [H][W][3] contiguous (the reference's storage order, functional.py:104-108) */

typedef struct sdsj_info {
    int32_t width, height; /* image size (PIL Image.size order: width, height) */
    int32_t ncomp;         /* 1 (grayscale), 3 (YCbCr; RGB-coded under SDSJ_FORMAT_JPEG_EXT) or, under
                              SDSJ_FORMAT_JPEG_CMYK, 4 (CMYK / YCCK) */
    int32_t h_samp[3], v_samp[3]; /* (of a four-component file: its first three components) */
    int32_t restart_interval;
    int32_t supported; /* 1 if the MI355X path decodes it */
    int64_t entropy_offset;
} sdsj_info;

typedef struct sdsj_cfg {
    int32_t abi_version;     /* must be SDSJ_ABI_VERSION */
    int32_t max_batch;       /* images per internal launch (0 = default 4096) */
    int64_t scratch_bytes;   /* device scratch capacity; 0 = grow on demand (host API) / 2 GiB */
} sdsj_cfg;

typedef struct sdsj_op {
    int32_t out_h, out_w;        /* target resolution, the reference's (h, w) tuple (functional.py:76) */
    int32_t crop_before_resize;  /* functional.py:45 (default 1): centre crop to out_w/out_h first */
    int32_t filter;              /* SDSJ_FILTER_*; the reference default is bilinear (functional.py:48) */
    int32_t out_dtype;           /* SDSJ_DTYPE_* */
    int32_t layout;              /* SDSJ_LAYOUT_* */
} sdsj_op;

typedef struct sdsj_engine sdsj_engine;

int sdsj_abi_version(void);

/* Host-side header parse of one JPEG (no GPU needed). */
int sdsj_probe(const uint8_t* jpg, size_t n, sdsj_info* out);

/* The same for an engine whose format mask is `formats` (it must have SDSJ_FORMAT_JPEG): with
 * SDSJ_FORMAT_JPEG_EXT, SDSJ_FORMAT_JPEG_SCANS or SDSJ_FORMAT_JPEG_CMYK (below) the files those bits admit are `supported`; without
 * them the result is sdsj_probe's. */
int sdsj_probe_formats(const uint8_t* jpg, size_t n, int formats, sdsj_info* out);

/* Device scratch one JPEG needs for `op` (host planning, no GPU): *need = bytes (256-aligned share of
 * the engine's scratch).  Returns the header status (SDSJ_OK, SDSJ_UNSUPPORTED, SDSJ_CORRUPT); a
 * batch on the device-resident entry point needs the sum over its samples (sdsj_engine_reserve). */
int sdsj_plan_need(const uint8_t* jpg, size_t n, const sdsj_op* op, int64_t* need);

/* Sample formats an engine decodes natively (sdsj_engine_set_formats).  JPEG only by default; PNG is
 * opt-in: non-interlaced, bit depth 8, colour types 0, 2, 3, 4, 6, giving the pixels of
 * PIL.Image.open(...).convert("RGB") -- gray replicated, alpha dropped, tRNS ignored, palette indices
 * at or beyond the PLTE length black.  A PNG outside that subset (interlaced, other depths, APNG, chunks
 * this path does not know before the image data) reports SDSJ_UNSUPPORTED and a stream this path is
 * not sure PIL decodes to the same pixels SDSJ_CORRUPT; callers rerun both on PIL, as for JPEG.
 *
 * SDSJ_FORMAT_PNG_EXT (valid only together with SDSJ_FORMAT_PNG, SDSJ_EINVAL otherwise) widens the subset:
 * Adam7 interlace, every legal (colour type, bit depth) pair -- gray 1 / 2 / 4 scaled by 255 / 85 / 17,
 * palette 1 / 2 / 4, gray 16 clipped to 255 (PIL opens it as I;16), the high byte of gray + alpha, RGB
 * and RGBA 16 -- and, before the image data, eXIf and every ancillary chunk PIL has no handler for
 * (tIME, bKGD, sBIT, private ones; CRC checked).  APNG, iCCP, zTXt and iTXt stay SDSJ_UNSUPPORTED.
 * Without the bit nothing changes: those files report SDSJ_UNSUPPORTED.
 *
 * SDSJ_FORMAT_PNG_META (valid only together with SDSJ_FORMAT_PNG, SDSJ_EINVAL otherwise; it may be combined
 * with SDSJ_FORMAT_PNG_EXT) accepts files as converters and editors write them: iCCP, zTXt and iTXt chunks
 * -- none changes a pixel of convert("RGB") -- and chunks after the image data (tEXt, gAMA, cHRM, sRGB,
 * pHYs, iCCP, zTXt, iTXt; with SDSJ_FORMAT_PNG_EXT also eXIf and the ancillary chunks PIL has no handler
 * for).  A compressed chunk is accepted only where its zlib stream is well formed and inflates to fewer than
 * 1,048,576 bytes (PIL raises above that), the text chunks of a file only up to 67,108,864 bytes in all
 * (PIL's limit); everything else, and APNG, stays SDSJ_UNSUPPORTED.  Without the bit nothing changes.
 *
 * SDSJ_FORMAT_JPEG_EXT (valid only together with SDSJ_FORMAT_JPEG, SDSJ_EINVAL otherwise; it combines freely
 * with the PNG bits) widens the three-component JPEG subset, baseline and progressive alike: every
 * sampling whose factors divide the largest (upsampling ratios 1..4 per axis and component: 4:1:1, 4:1:0,
 * 1x4, 3x1, 2x3, 2x4, a subsampled first component, mixed ratios; at most 10 blocks per MCU as before),
 * upsampled as libjpeg's jinit_upsampler chooses per component (fancy h2v1 / h2v2 / h1v2 as before, every
 * other ratio by replication, int_upsample), and RGB-coded files -- those libjpeg's
 * default_decompress_parms takes as JCS_RGB: no JFIF marker and an Adobe marker with transform 0, or
 * neither marker and the component ids 'R', 'G', 'B' -- whose planes are stored as R, G, B without a
 * colour transform.  Fractional ratios, four components (CMYK / YCCK: SDSJ_FORMAT_JPEG_CMYK), arithmetic and
 * 12-bit files stay SDSJ_UNSUPPORTED.  Without the bit nothing changes: those files report SDSJ_UNSUPPORTED.
 *
 * SDSJ_FORMAT_JPEG_SCANS (valid only together with SDSJ_FORMAT_JPEG, SDSJ_EINVAL otherwise; it combines freely
 * with SDSJ_FORMAT_JPEG_EXT and the PNG bits) accepts multi-scan sequential files: 8-bit SOF0 / SOF1 frames of
 * three components whose components arrive in more than one scan (Y, Cb, Cr one after another, Y then
 * Cb + Cr, any order and grouping; jpegtran -scans writes them), with or without restart intervals, with
 * DHT / DQT / DRI segments between the scans, each component's quantisation table latched at its first scan.
 * Every scan must be a full sequential one (Ss = 0, Se = 63, Ah = Al = 0) and code components no earlier scan
 * coded: a file that breaks either rule reports SDSJ_UNSUPPORTED (libjpeg only warns and overlays the
 * coefficients), a scan without restart intervals that holds fill bytes before a stuffed zero SDSJ_CORRUPT.
 * A file that ends at EOI before every component was coded decodes, the missing components from zero
 * coefficients, as in PIL.  Samplings with ratios of 3 and 4 and RGB-coded files need SDSJ_FORMAT_JPEG_EXT as
 * well.  Without the bit nothing changes: multi-scan sequential files report SDSJ_UNSUPPORTED.
 *
 * SDSJ_FORMAT_JPEG_CMYK (valid only together with SDSJ_FORMAT_JPEG, SDSJ_EINVAL otherwise; it combines freely
 * with every other bit) accepts four-component files: 8-bit sequential (SOF0 / SOF1) Huffman frames of four
 * components, giving the pixels of PIL.Image.open(...).convert("RGB").  The colour space is libjpeg's
 * default_decompress_parms choice -- an Adobe marker with transform 0, or no Adobe marker: CMYK; an Adobe marker
 * with any other transform: YCCK, whose first three planes are converted as ycck_cmyk_convert does; a JFIF
 * marker plays no part and the component ids are free -- and the samples are taken inverted, as Pillow takes
 * every four-component JPEG (Adobe's convention), then through Pillow's CMYK -> RGB.  Sampling factors are as
 * for three components: ratios of 1 and 2 with this bit alone (a subsampled first component, and a subsampled
 * K, included), ratios of 3 and 4 with SDSJ_FORMAT_JPEG_EXT as well; fractional ratios and more than 10 blocks
 * per MCU stay SDSJ_UNSUPPORTED / SDSJ_CORRUPT as before.  One interleaved scan of all four components decodes
 * with this bit alone; components that arrive in several scans need SDSJ_FORMAT_JPEG_SCANS as well and follow
 * its rules.  Restart intervals are supported.  Progressive (SOF2: SDSJ_FORMAT_JPEG_CMYK_PROG), arithmetic-coded
 * and 12-bit four-component files stay SDSJ_UNSUPPORTED.  Without the bit nothing changes: a four-component file
 * reports SDSJ_UNSUPPORTED on every entry point.
 *
 * SDSJ_FORMAT_JPEG_CMYK_PROG (valid only together with SDSJ_FORMAT_JPEG and SDSJ_FORMAT_JPEG_CMYK, SDSJ_EINVAL
 * otherwise -- 1024, 1025 and 1536 among them; it combines freely with every other bit) accepts progressive
 * four-component files: 8-bit SOF2 Huffman frames of four components, as Pillow writes a CMYK image with
 * progressive=True, decoded as libjpeg decodes them -- DC and AC first and refinement scans, the DC ones
 * interleaved over up to four components, EOB runs, restart intervals, DHT / DQT / DRI between scans, block
 * smoothing of all four components when the file ends before its last scans.  Colour space, component ids and
 * sampling factors follow SDSJ_FORMAT_JPEG_CMYK's rules: the Adobe marker chooses CMYK or YCCK, ratios of 1 and 2
 * with this bit, ratios of 3 and 4 with SDSJ_FORMAT_JPEG_EXT as well, fractional ratios SDSJ_UNSUPPORTED, more
 * than 10 blocks per MCU SDSJ_CORRUPT.  SDSJ_FORMAT_JPEG_SCANS plays no part (a progressive file always has
 * several scans), and SDSJ_CTR_PROGRESSIVE counts these files, as every SOF2 file.  Arithmetic-coded and 12-bit
 * files stay SDSJ_UNSUPPORTED.  Without the bit nothing changes: a progressive four-component file reports
 * SDSJ_UNSUPPORTED on every entry point.
 *
 * SDSJ_FORMAT_GIF is a third base format (valid alone or with any other bit): GIF87a / GIF89a, the first
 * frame on the logical screen, giving the pixels of PIL.Image.open(...).convert("RGB") -- the local colour
 * table if there is one, else the global one, indices at or beyond its entries black, where a table that is
 * the identity grey ramp counts as none; without a table (index, index, index); pixels outside the frame rectangle in the colour of index
 * 0, or of the transparent index when a graphic-control extension before the image sets one; interlaced
 * frames; LZW minimum code sizes 2..8.  The blocks before the first image descriptor must be well formed
 * (graphic-control, comment, application and plain-text extensions are walked by their sub-blocks), the
 * frame non-empty and inside the screen; nothing after the frame's data is read.  A frame that leaves the
 * screen, another code size, a file without an image descriptor and an unknown block report
 * SDSJ_UNSUPPORTED; an empty screen or frame, a sub-block past the input, an end code or the end of the
 * data before the last pixel, a code above the next free entry and a first code after a clear that is no
 * literal report SDSJ_CORRUPT (PIL raises on the truncated ones).  Callers rerun both on PIL.  Without the
 * bit nothing changes: a GIF reports SDSJ_UNSUPPORTED.
 *
 * SDSJ_FORMAT_WEBP is a fourth base format (valid alone or with any other bit): lossless WebP (VP8L, RFC 9649),
 * giving the pixels of PIL.Image.open(...).convert("RGB"), which drops alpha without compositing -- a bare
 * RIFF / WEBP / VP8L file, or a VP8X file whose ICCP, EXIF, "XMP " and unknown chunks are skipped and whose
 * canvas equals the frame; chunks padded to even sizes, bytes after the RIFF size ignored.  The whole codec:
 * the four transforms (predictor modes 0..15, cross-colour, subtract-green, colour-indexing with 1..256
 * entries) in any order, each at most once; a colour cache of 1..11 bits; a meta-prefix image; simple and
 * normal prefix codes; LZ77 with the short distance codes.  Lossy files ("VP8 ", with or without ALPH),
 * animated ones (the VP8X flag, ANIM, ANMF), a canvas that differs from the frame, a non-zero version and a
 * main image of more than 256 prefix-code groups report SDSJ_UNSUPPORTED; a RIFF or chunk size past the
 * input, a reserved VP8X bit, a second image chunk, a repeated transform, an incomplete or over-subscribed
 * prefix code, a copy that starts before the first pixel or ends past the last, and any read beyond the
 * chunk's last byte report SDSJ_CORRUPT (PIL raises on them).  Callers rerun both on PIL.  Without the bit
 * nothing changes: a WebP reports SDSJ_UNSUPPORTED.
 *
 * SDSJ_FORMAT_TIFF is a fifth base format (valid alone or with any other bit): classic TIFF (II or MM; the first
 * IFD, wherever it lies), giving the pixels of PIL.Image.open(...).convert("RGB").  Strips only (RowsPerStrip of
 * any value or absent; StripOffsets / StripByteCounts as SHORTs or LONGs), PlanarConfiguration 1, FillOrder 1,
 * Orientation 1 or absent, 8 bits per sample: grey (photometric 0, inverted, or 1), palette (3, ColorMap of 3 x 256
 * SHORTs, the high byte of each), RGB (2), RGB with one extra sample whose ExtraSamples is 0 or 2 and grey (1) with one of kind 2 (dropped),
 * CMYK (5, through PIL's cmyk2rgb).  Compression 1 (none), 32773 (PackBits), 5 (LZW, MSB first with the early
 * change) and 8 / 32946 (Deflate, a zlib stream per strip); Predictor 1, or 2 with LZW and Deflate.  BigTIFF,
 * tiles, planar configuration 2, other sample sizes and formats, associated alpha, several extra samples, every other grey file with an extra sample (PIL has no mode for it), YCbCr /
 * CIELab / mask photometrics, JPEG / CCITT / other compressions, predictor 3, old-style LZW and orientations 2..8
 * report SDSJ_UNSUPPORTED; an IFD, a value or a strip past the input, unsorted or duplicate tags, a tag outside the short list checked against libtiff (or one of them with another
 * type or count), RowsPerStrip of 0x80000000..0xFFFFFFFE, strip arrays
 * that do not match the rows, a palette file without a ColorMap of 768 entries, and a strip that does not decode to
 * exactly its rows (or whose Adler-32 is wrong or missing) report SDSJ_CORRUPT.  Callers rerun both on PIL.
 * Without the bit nothing changes: a TIFF reports SDSJ_UNSUPPORTED. */
#define SDSJ_FORMAT_JPEG 1
#define SDSJ_FORMAT_PNG 2
#define SDSJ_FORMAT_PNG_EXT 4
#define SDSJ_FORMAT_PNG_META 16
#define SDSJ_FORMAT_JPEG_EXT 64
#define SDSJ_FORMAT_JPEG_SCANS 128
#define SDSJ_FORMAT_GIF 256 /* (bits 8 and 32 are not formats: SDSJ_EINVAL) */
#define SDSJ_FORMAT_JPEG_CMYK 512
#define SDSJ_FORMAT_JPEG_CMYK_PROG 1024
#define SDSJ_FORMAT_WEBP 4096 /* (bit 2048 is not a format either: SDSJ_EINVAL, alone and beside any other bit) */
#define SDSJ_FORMAT_TIFF 16384 /* (nor is bit 8192) */

typedef struct sdsj_png_info {
    int32_t width, height;
    int32_t bit_depth, color_type, interlace; /* IHDR fields */
    int32_t supported;                        /* 1 if the MI355X path decodes it (when PNG is enabled) */
} sdsj_png_info;

/* Host-side header parse of one PNG up to its first IDAT chunk (no GPU needed): IHDR fields as soon as
 * IHDR is readable, and the status k_parse would give the sample with SDSJ_FORMAT_PNG enabled. */
int sdsj_png_probe(const uint8_t* png, size_t n, sdsj_png_info* out);

/* The same for an engine whose format mask is `formats` (it must have SDSJ_FORMAT_PNG): with
 * SDSJ_FORMAT_PNG_EXT the wider subset is `supported`; without it the result is sdsj_png_probe's.  With
 * SDSJ_FORMAT_PNG_META the status is the one the sample has before its image data is inflated: the
 * compressed chunks and the chunks after the image data are judged too (the whole file is walked). */
int sdsj_png_probe_formats(const uint8_t* png, size_t n, int formats, sdsj_png_info* out);

typedef struct sdsj_gif_info {
    int32_t width, height;                      /* the logical screen: the image's size */
    int32_t frame_x, frame_y, frame_w, frame_h; /* the first image descriptor's rectangle */
    int32_t interlace;
    int32_t table_entries; /* entries of the effective colour table; 0: grey (no table, or the identity ramp) */
    int32_t min_code_size; /* LZW minimum code size */
    int32_t supported;     /* 1 if the MI355X path decodes it (when GIF is enabled) */
} sdsj_gif_info;

/* Host-side parse of one GIF up to its first data sub-block (no GPU needed): the screen's size as soon as
 * it is readable, the other fields once the first image descriptor has been read, and the status k_parse
 * gives the sample with SDSJ_FORMAT_GIF enabled (the LZW data is the device's to judge). */
int sdsj_gif_probe(const uint8_t* gif, size_t n, sdsj_gif_info* out);

typedef struct sdsj_webp_info {
    int32_t width, height; /* the image's size: the VP8L or VP8 frame's, or the VP8X canvas while no frame was met */
    int32_t has_alpha;     /* the VP8L header's alpha bit or the VP8X alpha flag (convert("RGB") drops alpha) */
    int32_t lossless;      /* 1: VP8L, 0: VP8 (lossy) or no image chunk */
    int32_t extended;      /* 1: a VP8X file */
    int32_t supported;     /* 1 if the MI355X path decodes it (when WebP is enabled) */
} sdsj_webp_info;

/* Host-side parse of one WebP's container and VP8L header (no GPU needed): the size as soon as it is
 * readable -- of a lossy file too, which stays SDSJ_UNSUPPORTED --, and the status k_parse gives the sample
 * with SDSJ_FORMAT_WEBP enabled (the prefix-coded data is the device's to judge). */
int sdsj_webp_probe(const uint8_t* webp, size_t n, sdsj_webp_info* out);

typedef struct sdsj_tiff_info {
    int32_t width, height;   /* ImageWidth / ImageLength, as soon as they have been read */
    int32_t samples;         /* samples per pixel as stored (an extra sample included) */
    int32_t photometric;     /* 0, 1, 2, 3 or 5 */
    int32_t codec;           /* 1: none, 2: PackBits, 3: LZW, 4: Deflate */
    int32_t predictor;       /* 1 or 2 */
    int32_t rows_per_strip;  /* at most the height */
    int32_t strips;
    int32_t supported;       /* 1 if the MI355X path decodes it (when TIFF is enabled) */
} sdsj_tiff_info;

/* Host-side parse of one TIFF's header, first IFD and strip ranges (no GPU needed): the size as soon as it is
 * readable, and the status k_parse gives the sample with SDSJ_FORMAT_TIFF enabled (the strips' data is the
 * device's to judge).  The fields after the size are filled only for a supported file. */
int sdsj_tiff_probe(const uint8_t* tiff, size_t n, sdsj_tiff_info* out);

/* sdsj_plan_need for an engine whose format mask is `formats`: also sizes PNG samples when the mask
 * has SDSJ_FORMAT_PNG, GIF samples when it has SDSJ_FORMAT_GIF, WebP samples when it has SDSJ_FORMAT_WEBP and TIFF samples when it has SDSJ_FORMAT_TIFF (a format outside the mask reports
 * SDSJ_UNSUPPORTED, need 0).  With
 * SDSJ_FORMAT_JPEG_SCANS a multi-scan sequential file that is refused over its scans (not its header: a scan that
 * is not a sequential one, a component coded twice, fill bytes before a stuffed zero) reports that status together
 * with the bytes the device plans for it before it refuses it: a batch that holds the file needs them. */
int sdsj_plan_need_formats(const uint8_t* img, size_t n, const sdsj_op* op, int formats, int64_t* need);

/* Creates an engine bound to HIP device `hip_device`.  Scratch memory is owned by the engine.  An engine
 * takes one host call at a time: callers with several threads use one engine each, as the decode service does. */
int sdsj_engine_create(int hip_device, const sdsj_cfg* cfg, sdsj_engine** out);
int sdsj_engine_destroy(sdsj_engine* eng);

/* Sets the formats (SDSJ_FORMAT_* mask, at least one of JPEG, PNG, GIF, WEBP and TIFF) the engine decodes in batches submitted after the
 * call, on every decode entry point: sdsj_decode_resize_batch, sdsj_decode_resize_batch_device,
 * sdsj_submit_batch, sdsj_submit_files (and so what sdsj_wait_batch reports).  Default: JPEG only. */
int sdsj_engine_set_formats(sdsj_engine* eng, int mask);

/* Decode + crop + resize (+flip, +normalise) of n JPEGs held in HOST memory.
 *   jpg[i], len[i]  : encoded bytes of sample i (borrowed)
 *   flip            : host array of n bytes (1 = horizontal flip) or NULL
 *   out             : device pointer to n * out_h * out_w * 3 elements of op->out_dtype, laid
 *                     out per op->layout, sample-major; allocated by the caller (torch).  Pinned
 *                     host memory (hipHostMalloc / torch pin_memory) is device-accessible and works
 *                     too: the kernels then store the pixels over PCIe (no separate D2H copy)
 *   status          : host array of n ints, per-sample SDSJ_* code (filled before return)
 * Synchronises `hip_stream` before returning (status is host memory). */
int sdsj_decode_resize_batch(sdsj_engine* eng, int n, const uint8_t* const* jpg, const size_t* len,
                             const sdsj_op* op, const uint8_t* flip, void* out, int32_t* status,
                             void* hip_stream);

/* Same with inputs already in DEVICE memory: sample i is d_blob[d_offsets[i] .. + d_lengths[i]) of the
 * blob_bytes-byte buffer d_blob; a sample whose range is negative or leaves the buffer reports
 * SDSJ_EINVAL (checked on the device before anything reads it).  d_flip (n bytes) may be NULL;
 * d_status is a device array of n ints.  Fully asynchronous on `hip_stream` (no host
 * synchronisation, capturable into a hipGraph for a fixed n). */
int sdsj_decode_resize_batch_device(sdsj_engine* eng, int n, const uint8_t* d_blob, size_t blob_bytes,
                                    const int64_t* d_offsets, const int32_t* d_lengths, const sdsj_op* op,
                                    const uint8_t* d_flip, void* d_out, int32_t* d_status, void* hip_stream);

/* Asynchronous host path with double-buffered pinned staging (downloader /
 * host cache -> pinned staging -> H2D -> decode, overlapped; config 5).  Up to SDSJ_SLOTS batches are
 * in flight.  A submit stages its batch into the slot's pinned buffer -- while the GPU still decodes
 * the previous batch --, copies it H2D on an engine-owned copy stream and enqueues the decode on
 * `hip_stream` behind that copy, then returns.  sdsj_wait_batch blocks until the slot's batch is done
 * and fills its per-sample status.  `out` (device, as in sdsj_decode_resize_batch) must stay untouched
 * until then.  n <= the engine's max_batch.  Submitting to a slot still in flight waits for it first
 * (its statuses are then dropped).
 *   sdsj_submit_batch : encoded bytes in host memory, borrowed for the call only
 *                       (same samples as sdsj_decode_resize_batch)
 *   sdsj_submit_files : n file paths read straight into the slot's pinned buffer -- what
 *                       LoadFromDiskTransform (presets.py:613-626) does with the local cache that
 *                       run_downloading_task (downloader.py:117-131) fills.  A file that cannot be
 *                       read is reported per sample as SDSJ_EINVAL. */
#define SDSJ_SLOTS 2
int sdsj_submit_batch(sdsj_engine* eng, int slot, int n, const uint8_t* const* jpg, const size_t* len,
                      const sdsj_op* op, const uint8_t* flip, void* out, void* hip_stream);
int sdsj_submit_files(sdsj_engine* eng, int slot, int n, const char* const* paths, const sdsj_op* op,
                      const uint8_t* flip, void* out, void* hip_stream);
int sdsj_wait_batch(sdsj_engine* eng, int slot, int32_t* status);

/* Crop + resize (+flip, +normalise) of n raw RGB frames already in DEVICE memory -- the video path
 * (sds/transforms/presets.py:121-135 ResizeVideoTransform + ConvertVideoToByteTensorTransform ->
 * functional.py:42-86 lean_resize_frames on the frames PyAV decoded).  Frame i is uint8 HWC
 * [height][width][3] at d_frames + i * frame_stride (frame_stride >= width * height * 3).  Same
 * op, flip, output and status conventions as sdsj_decode_resize_batch_device.  Synchronises
 * `hip_stream` between chunks of max_batch frames (host-planned descriptors are staged). */
int sdsj_resize_frames_device(sdsj_engine* eng, int n, const uint8_t* d_frames, int32_t width, int32_t height,
                              int64_t frame_stride, const sdsj_op* op, const uint8_t* d_flip, void* d_out,
                              int32_t* d_status, void* hip_stream);

/* Per-process counters (SURVEY.md §5 metrics; sds itself only logs through loguru, sds/__init__.py:5-17).
 * Accumulated on the device by every batch an engine decodes, over all entry points: samples by
 * status, encoded bytes in, output bytes out.  sdsj_engine_counters waits for the work queued so far
 * and copies up to `cap` counters (index = SDSJ_CTR_*); `reset` != 0 zeroes them afterwards. */
#define SDSJ_CTR_IMAGES 0      /* JPEG samples submitted */
#define SDSJ_CTR_OK 1          /* samples (images or frames) decoded / resized */
#define SDSJ_CTR_UNSUPPORTED 2 /* valid images this path does not decode (PNG, WebP, arithmetic, 12-bit, CMYK without its bit...) */
#define SDSJ_CTR_CORRUPT 3     /* malformed / truncated streams */
#define SDSJ_CTR_CAPACITY 4    /* samples that did not fit the scratch */
#define SDSJ_CTR_OTHER 5       /* other per-sample errors (unreadable files) */
#define SDSJ_CTR_BYTES_IN 6    /* encoded bytes of the JPEG samples */
#define SDSJ_CTR_BYTES_OUT 7   /* output tensor bytes written (failed samples included: zeros) */
#define SDSJ_CTR_FRAMES 8      /* raw frames resized (sdsj_resize_frames_device) */
#define SDSJ_CTR_PROGRESSIVE 9 /* progressive JPEGs decoded */
#define SDSJ_CTR_PNG 10        /* PNG samples decoded natively (SDSJ_FORMAT_PNG and its _EXT / _META bits) */
#define SDSJ_NUM_COUNTERS 11
int sdsj_engine_counters(sdsj_engine* eng, uint64_t* out, int cap, int reset);
const char* sdsj_counter_name(int k);

/* Entry-point store.  The device-resident entry point keeps, per row it has decoded -- keyed by the sample's
 * device address --, the entry state of every entropy subsequence, and on a later call over the same bytes
 * skips the speculative and sync passes that compute them: a dataset resident in device memory is decoded
 * epoch after epoch.  The write pass proves every stored state while it decodes and falls back to the full
 * decode in the same call, so a sample replaced in place costs time and never pixels.  It serves baseline images
 * of the single-workgroup 11-bit route; the host entry points never use it.
 * sdsj_engine_set_hints: rows the store holds (default 2 x max_batch, about 4.2 KB of device memory each,
 * allocated on the first device-resident call; 0 turns the store off, as the environment's SDSJ_HINTS=0 does);
 * waits for the device, and empties the store.  sdsj_engine_clear_hints empties it.
 * sdsj_engine_hint_counters: as sdsj_engine_counters, for the store's own counters (SDSJ_HINT_CTR_*). */
#define SDSJ_HINT_CTR_HITS 0          /* images decoded from stored entry states, proved by the write pass */
#define SDSJ_HINT_CTR_MISSES 1        /* eligible images without a usable record */
#define SDSJ_HINT_CTR_VERIFY_FAILED 2 /* images whose record the write pass refuted (decoded again in the call) */
#define SDSJ_HINT_CTR_STORED 3        /* records written */
#define SDSJ_NUM_HINT_COUNTERS 4
int sdsj_engine_set_hints(sdsj_engine* eng, int64_t rows);
int sdsj_engine_clear_hints(sdsj_engine* eng);
int sdsj_engine_hint_counters(sdsj_engine* eng, uint64_t* out, int cap, int reset);
const char* sdsj_hint_counter_name(int k);

/* Kernel lanes: a batch of >= 256 x L images runs as L contiguous lanes on L streams whose kernel
 * sequences overlap (default 4, at most 4).  1 = one dispatch of every kernel per batch, the setting
 * under which a kernel's launch duration is measured alone (bench.py roofline). */
int sdsj_engine_set_lanes(sdsj_engine* eng, int lanes);

/* Grows the engine's device scratch to at least `bytes` (waits for the device first).  The device-resident
 * entry point never grows scratch by itself (it does not synchronise): its capacity is the engine's
 * cfg->scratch_bytes, or 2 GiB at the first call; samples beyond it report SDSJ_ECAPACITY. */
int sdsj_engine_reserve(sdsj_engine* eng, int64_t bytes);

/* Stage timing: sdsj_engine_set_timing(e, 1) starts (and restarts) accumulation; every chunk launched
 * afterwards records HIP events around each kernel on the caller's stream.  sdsj_engine_stage_times
 * waits for the last recorded chunk and returns, per stage, the summed device milliseconds. */
int sdsj_engine_set_timing(sdsj_engine* eng, int enable);
int sdsj_engine_stage_times(const sdsj_engine* eng, float* ms, int cap, int* n_stages);

const char* sdsj_last_error(const sdsj_engine* eng);

/* Node-local decode service (SURVEY.md §8(f) f1 for the reference's own loader shape: sds runs the
 * transform list per sample inside forked DataLoader workers, sds/dataset.py:535-561, with
 * DataLoader(num_workers=2, pin_memory=True), examples/iter_image_dataset.py:72-80 /
 * sds/dataloader.py:191-193 -- workers that cannot initialise HIP after their parent did).  One
 * process per GPU owns `engines` engines (each its own stream and scratch, one batch in flight each);
 * the per-sample transform in every worker sends its encoded bytes through a shared-memory region and
 * a SOCK_SEQPACKET request, and the service coalesces the requests of all workers into batched engine
 * calls and writes host outputs (the reference's tensor type) back into the worker's region.
 *
 * Wire protocol (little-endian, fixed-size packets on an AF_UNIX SOCK_SEQPACKET connection):
 *   client -> service  sdsj_svc_req.  kind MAP carries the client's region (memfd) as SCM_RIGHTS, in_len =
 *                      its size; the service maps it and replies.  kind DECODE: the JPEG is region[0,
 *                      in_len), the output (op->out_h * out_w * 3 elements of op->out_dtype, op->layout) is
 *                      written to region[out_off, ...).  kind FRAME: region[0, in_len) is a uint8 HWC RGB
 *                      frame of width x height (a sample decoded by PIL), cropped / resized as DECODE does.
 *   service -> client  sdsj_svc_rep {seq, status}: status = the sample's SDSJ_* code (the output is in the
 *                      region when SDSJ_OK). */
#define SDSJ_SVC_MAGIC 0x4A534453u /* "SDSJ" */
#define SDSJ_SVC_MAP 1
#define SDSJ_SVC_DECODE 2
#define SDSJ_SVC_FRAME 3
typedef struct sdsj_svc_req {
    uint32_t magic, kind;
    uint64_t seq;
    int64_t in_len, out_off;
    int32_t width, height; /* FRAME only */
    sdsj_op op;
    int32_t flip;
    int32_t reserved;
} sdsj_svc_req; /* 72 bytes */
typedef struct sdsj_svc_rep {
    uint64_t seq;
    int32_t status, reserved;
} sdsj_svc_rep; /* 16 bytes */

typedef struct sdsj_service_cfg {
    int32_t abi_version; /* SDSJ_ABI_VERSION */
    int32_t device;      /* HIP device */
    int32_t engines;     /* batches in flight at once (0 = 8) */
    int32_t max_batch;   /* requests per batch (0 = 64) */
    int32_t listen_fd;   /* a bound, listening AF_UNIX SOCK_SEQPACKET socket */
    int32_t parent_pid;  /* the service returns when this process is gone (0 = never) */
} sdsj_service_cfg;

/* Serves requests until SIGTERM / SIGINT or the parent's exit; returns SDSJ_OK, or an error code with a
 * message on stderr.  Runs in the calling thread (the service process's main thread). */
int sdsj_service_serve(const sdsj_service_cfg* cfg);

/* Diagnostics for tests: device pointers of the engine's scratch and per-image descriptor array of the
 * most recent chunk, and the byte size of one descriptor (layout: sds_amd/csrc/sdsj_common.h ImgDesc). */
int sdsj_engine_debug_buffers(const sdsj_engine* eng, void** scratch, void** descs, int64_t* desc_bytes,
                              int64_t* scratch_bytes);

/* Name of stage k of sdsj_engine_stage_times ("parse", "unstuff", "entropy", ...; the PNG kernels'
 * "png_inflate" and "png_unfilter" come last, though they run after "prog"). */
const char* sdsj_stage_name(int k);

#ifdef __cplusplus
}
#endif
#endif /* SDSJ_H */
