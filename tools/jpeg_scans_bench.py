"""Throughput of the opt-in multi-scan sequential JPEG route (gpu_formats "jpeg-scans": k_scans walks a file's scans
with one wave) next to the route it replaces, decode + resize to 256x256 of one pool of 640x480 4:2:0 files:

  8 distinct images: synth_rgb -> YCbCr -> chroma averaged over 2 x 2 -> a numpy forward DCT ->
  tests/jpeg_scans_synth.write_multiscan as three scans, Y, Cb, Cr (Pillow writes no such file), replicated

One JSON line per route, each measured once (marked "single_run"):

  native     device-resident, formats=("jpeg", "jpeg-scans")               (argv[1] images per call, default 4096)
  control    the same coefficients as one interleaved scan (tests/jpeg_ext_synth.write_baseline), device-resident
             under the default mask: what the baseline entropy kernels make of the same images
  fallback   the default route for the multi-scan samples: GpuDecodeBatch with gpu_formats=("jpeg",), every sample
             decoded by PIL in the calling process and resized on the GPU  (at most 512 images)
  latency    one-image calls through the per-sample transform, native and default route (ms per image)

The native line carries PIL's rate on 16 cores over the pool's files.  The lines are printed and appended to --out
(default profiles/jpeg_scans_bench.jsonl).  `python tools/jpeg_scans_bench.py [N] [route ...] [--out FILE]`."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

SCANS = ("jpeg", "jpeg-scans")


def make_pools(count=8):
    """(three-scan files, the same coefficients as one interleaved scan) of natural-looking 4:2:0 content."""
    import numpy as np

    from jpeg_ext_bench import _dct_matrix
    from tests import jpeg_ext_synth as J
    from tests import jpeg_scans_synth as S
    from tests.golden.coefjpeg import ZIGZAG_TO_NATURAL
    from tests.golden.synth import synth_rgb
    w, h, samp = 640, 480, S.SETS["420"]
    m = _dct_matrix()
    u, v = np.mgrid[0:8, 0:8]
    qnat = [4 + 2 * (u + v), 6 + 3 * (u + v)]  # natural order; luma, chroma
    q = {t: qnat[t].reshape(64)[ZIGZAG_TO_NATURAL] for t in range(2)}
    multi, single = [], []
    for i in range(count):
        rgb = synth_rgb(np.random.default_rng(4321 + i), w, h).astype(np.float64)
        r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
        planes = [0.299 * r + 0.587 * g + 0.114 * b,
                  (-0.168736 * r - 0.331264 * g + 0.5 * b + 128).reshape(h // 2, 2, w // 2, 2).mean((1, 3)),
                  (0.5 * r - 0.418688 * g - 0.081312 * b + 128).reshape(h // 2, 2, w // 2, 2).mean((1, 3))]
        blocks = []
        for ci, p in enumerate(planes):  # (640 x 480 is a whole number of 16 x 16 MCUs: no padding blocks)
            bh, bw = p.shape[0] // 8, p.shape[1] // 8
            blk = (p - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
            coef = np.rint(m @ blk @ m.T / qnat[0 if ci == 0 else 1]).astype(np.int64)
            blocks.append(coef.reshape(bh, bw, 64)[..., ZIGZAG_TO_NATURAL])
        multi.append(S.write_multiscan(w, h, samp, blocks, q, S.GROUPS["y-cb-cr"]))
        single.append(J.write_baseline(w, h, samp, blocks, q))
    return multi, single


def main():
    import jpeg_ext_bench as E
    args = sys.argv[1:]
    out = os.path.join(REPO, "profiles", "jpeg_scans_bench.jsonl")
    if "--out" in args:
        k = args.index("--out")
        out = args[k + 1]
        del args[k:k + 2]
    n = int(args[0]) if args else 4096
    routes = args[1:] or ["native", "control", "fallback", "latency"]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    multi, single = make_pools()
    case = "4:2:0 as three scans (Y, Cb, Cr)"
    run = {"native": lambda: E.native(multi, n, case, SCANS),
           "control": lambda: dict(E.native(single, n, "4:2:0, the same coefficients as one interleaved scan", ("jpeg",)),
                                   route="control"),
           "fallback": lambda: E.fallback(multi, n, case),
           "latency": lambda: E.latency(multi, n, case, SCANS)}
    for r in routes:
        line = run[r]()
        line["single_run"] = True
        text = json.dumps(line)
        print(text, flush=True)
        with open(out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
