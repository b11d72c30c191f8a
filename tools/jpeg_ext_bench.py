"""Throughput of the opt-in wider JPEG subset (gpu_formats "jpeg-ext": k_color's int_upsample and the RGB-coded
store, through the unfused colour / resample passes) next to the route it replaces, decode + resize to 256x256 of
two pools of 640x480 files:

  4:1:1       8 distinct images: synth_rgb -> YCbCr -> chroma averaged over 4 columns -> a numpy forward DCT ->
              tests/jpeg_ext_synth.write_baseline (Pillow writes no 4:1:1), replicated
  RGB-coded   64 distinct images saved by Pillow with keep_rgb=True (quality 90)

One JSON line per pool and route, each measured once (marked "single_run"):

  native     device-resident, formats=("jpeg", "jpeg-ext")                 (argv[1] images per call, default 4096)
  fallback   the default route for the same samples: GpuDecodeBatch with gpu_formats=("jpeg",), every sample
             decoded by PIL in the calling process and resized on the GPU  (at most 512 images)
  latency    one-image calls through the per-sample transform, native and default route (ms per image)

`--controls` measures two other pools instead, to say where the RGB-coded pool's time goes: its images saved as
ordinary YCbCr 4:4:4 at quality 90 (default subset, fused route), and RGB-coded at quality 75; native route only.

The lines are printed and appended to --out (default profiles/jpeg_ext_bench.jsonl).
`python tools/jpeg_ext_bench.py [N] [route ...] [--controls] [--out FILE]`."""
import io
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

EXT = ("jpeg", "jpeg-ext")
RES = (256, 256)


def _dct_matrix():
    import numpy as np
    k, x = np.mgrid[0:8, 0:8]
    m = np.cos((2 * x + 1) * k * np.pi / 16) / 2
    m[0] /= np.sqrt(2)
    return m  # orthonormal: coefficients = m @ block @ m.T


def make_411_pool(count=8):
    """4:1:1 files (Y 4x1, Cb 1x1, Cr 1x1) of natural-looking content, written from forward-DCT coefficients."""
    import numpy as np

    from tests import jpeg_ext_synth as J
    from tests.golden.coefjpeg import ZIGZAG_TO_NATURAL
    from tests.golden.synth import synth_rgb
    w, h, samp = 640, 480, J.SETS["411"]
    m = _dct_matrix()
    u, v = np.mgrid[0:8, 0:8]
    qnat = [4 + 2 * (u + v), 6 + 3 * (u + v)]  # natural order; luma, chroma
    q = {t: qnat[t].reshape(64)[ZIGZAG_TO_NATURAL] for t in range(2)}
    pool = []
    for i in range(count):
        rgb = synth_rgb(np.random.default_rng(4321 + i), w, h).astype(np.float64)
        r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
        planes = [0.299 * r + 0.587 * g + 0.114 * b,
                  (-0.168736 * r - 0.331264 * g + 0.5 * b + 128).reshape(h, w // 4, 4).mean(-1),
                  (0.5 * r - 0.418688 * g - 0.081312 * b + 128).reshape(h, w // 4, 4).mean(-1)]
        blocks = []
        for ci, p in enumerate(planes):  # (640 x 480 is a whole number of 32 x 8 MCUs: no padding blocks)
            bh, bw = p.shape[0] // 8, p.shape[1] // 8
            blk = (p - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
            coef = np.rint(m @ blk @ m.T / qnat[0 if ci == 0 else 1]).astype(np.int64)
            blocks.append(coef.reshape(bh, bw, 64)[..., ZIGZAG_TO_NATURAL])
        pool.append(J.write_baseline(w, h, samp, blocks, q))
    return pool


def make_rgb_pool(count=64, **save):
    """The pool's images saved by Pillow: RGB-coded at quality 90 unless `save` says otherwise."""
    import numpy as np
    from PIL import Image

    from tests.golden.synth import synth_rgb
    save = save or dict(quality=90, keep_rgb=True)
    pool = []
    for i in range(count):
        b = io.BytesIO()
        Image.fromarray(synth_rgb(np.random.default_rng(1234 + i), 640, 480)).save(b, "JPEG", **save)
        pool.append(b.getvalue())
    return pool


def native(pool, n, case, formats=EXT):
    import numpy as np
    import torch

    import bench
    from sds_amd.engine import JpegEngine
    jpgs = [pool[i % len(pool)] for i in range(n)]
    lens = [len(j) for j in jpgs]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    blob = torch.from_numpy(np.frombuffer(b"".join(jpgs), np.uint8).copy()).cuda()  # HBM-resident
    d_offs, d_lens = torch.from_numpy(offs).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    need = JpegEngine.scratch_need(pool, RES, formats=formats) * ((n + len(pool) - 1) // len(pool))
    eng = JpegEngine(max_batch=n, scratch_bytes=need + (64 << 20))
    out, st = eng.decode_resize_device(blob, d_offs, d_lens, RES, formats=formats)
    torch.cuda.synchronize()
    assert (st == 0).all(), st[st != 0][:8]
    assert eng.counters()["ok"] == n
    t0 = time.perf_counter()
    for _ in range(3):
        eng.decode_resize_device(blob, d_offs, d_lens, RES, out=out, status=st, formats=formats)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    eng.set_timing(True)
    eng.decode_resize_device(blob, d_offs, d_lens, RES, out=out, status=st, formats=formats)
    stages = {k: round(v, 3) for k, v in eng.stage_times().items() if v > 0.0005}
    eng.set_timing(False)
    folder = tempfile.mkdtemp()
    paths = []
    for i, j in enumerate(pool):  # the CPU baseline reads files (LoadFromDiskTransform)
        paths.append(os.path.join(folder, f"{i:03d}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(j)
    procs = min(16, bench.host_cores())
    cpu1 = bench.cpu_baseline(paths, 1, 2.0)
    cpup = bench.cpu_baseline(paths, procs, 4.0)
    return {"route": "native", "case": case,
            "metric": f"images/s JPEG 640x480 {case} decode+resize@256 (device-resident, gpu_formats {formats[-1]})",
            "value": round(n / dt, 1), "batch": n, "calls_timed": 3, "distinct_images": len(pool),
            "mean_jpeg_bytes": round(float(np.mean(lens)), 1), "stage_ms": stages,
            "cpu_baseline": {"value": round(cpup, 1), "cores": procs, "single_core_value": round(cpu1, 1),
                             "kind": "reference", "sample": "PIL open+convert, crop, BILINEAR 256x256, CHW tensor "
                             "over the pool's files"}}


def fallback(pool, n, case):
    import torch

    from sds_amd.batched import GpuDecodeBatch
    from sds_amd.engine import get_engine
    n = min(n, 512)
    jpgs = [pool[i % len(pool)] for i in range(n)]
    dec = GpuDecodeBatch("jpg", RES, device="cuda")
    dec({"jpg": jpgs[:64]})
    torch.cuda.synchronize()
    c0 = get_engine("cuda").counters()
    t0 = time.perf_counter()
    dec({"jpg": jpgs})
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert get_engine("cuda").counters()["fallback"] - c0["fallback"] == n
    return {"route": "fallback", "case": case,
            "metric": f"images/s JPEG 640x480 {case}, GpuDecodeBatch default gpu_formats (PIL decode per sample in "
            "the calling process, resize on the GPU)", "value": round(n / dt, 1), "batch": n}


def latency(pool, n, case, formats=EXT):
    import torch

    from sds_amd.presets import create_standard_image_pipeline
    folder = tempfile.mkdtemp()
    paths = []
    for i, j in enumerate(pool[:16]):
        paths.append(os.path.join(folder, f"{i:03d}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(j)
    res = {}
    for name, fm in (("native_ms", formats), ("default_route_ms", ("jpeg",))):
        ts = create_standard_image_pipeline("jpg", RES, device="cuda", service=None, gpu_formats=fm)
        for rep in range(2):  # (the first pass warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p in paths:
                s = {"jpg": p}
                for t in ts:
                    s = t(s)
            torch.cuda.synchronize()
            res[name] = round((time.perf_counter() - t0) / len(paths) * 1e3, 3)
    return {"route": "latency", "case": case,
            "metric": f"ms per one-image call, per-sample transform, JPEG 640x480 {case} -> 256x256", **res}


def main():
    args = sys.argv[1:]
    out = os.path.join(REPO, "profiles", "jpeg_ext_bench.jsonl")
    if "--out" in args:
        k = args.index("--out")
        out = args[k + 1]
        del args[k:k + 2]
    controls = "--controls" in args
    args = [a for a in args if a != "--controls"]
    n = int(args[0]) if args else 4096
    routes = args[1:] or (["native"] if controls else ["native", "fallback", "latency"])  # (the controls: native only)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if controls:  # where the RGB-coded pool's time goes: the same images as plain YCbCr 4:4:4, and RGB-coded at q75
        pools = (("YCbCr 4:4:4 q90 control", make_rgb_pool(quality=90, subsampling=0)),
                 ("RGB-coded q75", make_rgb_pool(quality=75, keep_rgb=True)))
    else:
        pools = (("4:1:1", make_411_pool()), ("RGB-coded", make_rgb_pool()))
    for case, pool in pools:
        for r in routes:
            line = {"native": native, "fallback": fallback, "latency": latency}[r](pool, n, case)
            line["single_run"] = True
            text = json.dumps(line)
            print(text, flush=True)
            with open(out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
