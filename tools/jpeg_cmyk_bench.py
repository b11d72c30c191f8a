"""Throughput of the opt-in four-component JPEG route (gpu_formats "jpeg-cmyk": k_scans walks the file's scan with one
wave, k_idct<4> and k_cmyk follow) next to the route it replaces, decode + resize to 256x256 of two pools of 640x480
files:

  CMYK   8 distinct images: synth_rgb -> convert("CMYK") -> Pillow's JPEG encoder at quality 90 (Adobe transform 0,
         no subsampling: what Pillow writes for a CMYK image), replicated
  YCCK   the same images as Photoshop-style YCCK: Y and K at full resolution, Cb and Cr averaged over 2 x 2 (sampling
         2x2, 1x1, 1x1, 2x2: 10 blocks per MCU) -> a numpy forward DCT -> tests/jpeg_cmyk_synth.write4 with an Adobe
         transform-2 marker, replicated

One JSON line per pool and route, each measured once (marked "single_run"):

  native     device-resident, formats=("jpeg", "jpeg-cmyk")                (argv[1] images per call, default 4096)
  fallback   the default route for the same samples: GpuDecodeBatch with gpu_formats=("jpeg",), every sample decoded
             by PIL in the calling process and resized on the GPU  (at most 512 images)
  latency    one-image calls through the per-sample transform, native and default route (ms per image)

The native line carries PIL's rate on 16 cores over the pool's files.  The lines are printed and appended to --out
(default profiles/jpeg_cmyk_bench.jsonl).  `python tools/jpeg_cmyk_bench.py [N] [route ...] [--out FILE]`.

--prog: the progressive pools of gpu_formats "jpeg-cmyk-prog" instead (k_prog4 walks the 18 scans Pillow writes for a
CMYK image with progressive=True), the same 8 images at quality 90 without subsampling and with subsampling=2;
native = formats ("jpeg-cmyk-prog",), the default route as above; --out defaults to
profiles/jpeg_cmyk_prog_bench.jsonl."""
import io
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

CMYK = ("jpeg", "jpeg-cmyk")
PROG = ("jpeg-cmyk-prog",)


def make_pools(count=8):
    """(Pillow-written CMYK files, writer-made YCCK 2x2,1x1,1x1,2x2 files) of the same natural-looking content."""
    import numpy as np
    from PIL import Image

    from jpeg_ext_bench import _dct_matrix
    from tests import jpeg_cmyk_synth as S
    from tests.golden.coefjpeg import ZIGZAG_TO_NATURAL
    from tests.golden.synth import synth_rgb
    w, h = 640, 480
    m = _dct_matrix()
    u, v = np.mgrid[0:8, 0:8]
    qnat = [4 + 2 * (u + v), 6 + 3 * (u + v)]  # natural order; first component, the others
    q = {t: qnat[t].reshape(64)[ZIGZAG_TO_NATURAL] for t in range(2)}
    cmyk, ycck = [], []
    for i in range(count):
        rgb8 = synth_rgb(np.random.default_rng(4321 + i), w, h)
        b = io.BytesIO()
        Image.fromarray(rgb8).convert("CMYK").save(b, "JPEG", quality=90)
        cmyk.append(b.getvalue())
        rgb = rgb8.astype(np.float64)
        r, g, bl = rgb[..., 0], rgb[..., 1], rgb[..., 2]
        planes = [0.299 * r + 0.587 * g + 0.114 * bl,
                  (-0.168736 * r - 0.331264 * g + 0.5 * bl + 128).reshape(h // 2, 2, w // 2, 2).mean((1, 3)),
                  (0.5 * r - 0.418688 * g - 0.081312 * bl + 128).reshape(h // 2, 2, w // 2, 2).mean((1, 3)),
                  255.0 - (255.0 - rgb.max(-1)) * 0.5]
        blocks = []
        for ci, p in enumerate(planes):  # (640 x 480 is a whole number of 16 x 16 MCUs: no padding blocks)
            bh, bw = p.shape[0] // 8, p.shape[1] // 8
            blk = (p - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
            coef = np.rint(m @ blk @ m.T / qnat[0 if ci == 0 else 1]).astype(np.int64)
            blocks.append(coef.reshape(bh, bw, 64)[..., ZIGZAG_TO_NATURAL])
        ycck.append(S.write4(w, h, S.S_PHOTOSHOP, blocks, q, lead=S.adobe(2)))
    return cmyk, ycck


def make_prog_pools(count=8):
    """(no subsampling, subsampling=2): progressive CMYK files as Pillow writes them, of make_pools' images."""
    import numpy as np
    from PIL import Image

    from tests.golden.synth import synth_rgb
    pools = ([], [])
    for i in range(count):
        img = Image.fromarray(synth_rgb(np.random.default_rng(4321 + i), 640, 480)).convert("CMYK")
        for pool, ss in zip(pools, (0, 2)):
            b = io.BytesIO()
            img.save(b, "JPEG", quality=90, progressive=True, subsampling=ss)
            pool.append(b.getvalue())
    return pools


def main():
    import jpeg_ext_bench as E
    args = sys.argv[1:]
    prog = "--prog" in args
    if prog:
        args.remove("--prog")
    out = os.path.join(REPO, "profiles", "jpeg_cmyk_prog_bench.jsonl" if prog else "jpeg_cmyk_bench.jsonl")
    if "--out" in args:
        k = args.index("--out")
        out = args[k + 1]
        del args[k:k + 2]
    n = int(args[0]) if args else 4096
    routes = args[1:] or ["native", "fallback", "latency"]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if prog:
        p0, p2 = make_prog_pools()
        pools = (("progressive CMYK as Pillow writes it (18 scans, quality 90, 1x1 sampling)", p0),
                 ("progressive CMYK as Pillow writes it (18 scans, quality 90, subsampling=2)", p2))
    else:
        cmyk, ycck = make_pools()
        pools = (("CMYK as Pillow writes it (Adobe transform 0, 1x1 sampling)", cmyk),
                 ("YCCK 2x2,1x1,1x1,2x2 (Adobe transform 2)", ycck))
    formats = PROG if prog else CMYK
    for case, pool in pools:
        run = {"native": lambda: E.native(pool, n, case, formats), "fallback": lambda: E.fallback(pool, n, case),
               "latency": lambda: E.latency(pool, n, case, formats)}
        for r in routes:
            line = run[r]()
            line["single_run"] = True
            text = json.dumps(line)
            print(text, flush=True)
            with open(out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
