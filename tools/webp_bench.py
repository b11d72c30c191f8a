"""Throughput of the opt-in native lossless WebP path (k_webp_decode, k_webp_inverse, k_webp_rgb) next to the
routes it replaces: a pool of 64 synthetic 640x480 photos (synth_rgb) written by Pillow as WebP with lossless=True
(libwebp's default method 4), decode + resize to 256x256.  One JSON line per route:

  native     device-resident, formats=("jpeg", "webp")                     (argv[1] images per call)
  fallback   the default route for the same samples: GpuDecodeBatch with gpu_formats=("jpeg",), every WebP
             decoded by PIL in the calling process and resized on the GPU  (at most 512 images)
  latency    one-image calls through the per-sample transform, native and default route (ms per image)
  mosaic     the native route on a second pool: 64 pictures of differently textured tiles (mosaic), which libwebp
             codes with tens of prefix-code groups, so the decode switches its tables every few pixels; with PIL on
             16 cores for the same files

The native line carries the pool's mean file size, bench.cpu_baseline over the pool written to files, on 1 and
16 cores, and the engine's stage times (the three WebP kernels run in the png_inflate slot).
`python tools/webp_bench.py N [route ...]`."""
import io
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WEBP = ("jpeg", "webp")


def make_pool():
    import numpy as np
    from PIL import Image

    from tests.golden.synth import synth_rgb
    pool = []
    for i in range(64):
        b = io.BytesIO()
        Image.fromarray(synth_rgb(np.random.default_rng(1234 + i), 640, 480)).save(b, "WEBP", lossless=True)
        pool.append(b.getvalue())
    return pool


def mosaic(rng, w, h, tile=32):
    """A picture of differently textured tiles (flat, ramps, stripes, noise of several strengths, blobs), as a real
    photograph has regions of different statistics: libwebp's encoder gives such a file tens of prefix-code groups,
    where a synth photo gets one or two."""
    import numpy as np
    out = np.zeros((h, w, 3), np.uint8)
    y, x = np.mgrid[0:tile, 0:tile]
    for ty in range(0, h, tile):
        for tx in range(0, w, tile):
            kind = int(rng.integers(0, 6))
            base = rng.integers(0, 256, 3)
            if kind == 0:
                t = np.broadcast_to(base, (tile, tile, 3)).astype(np.float64)
            elif kind == 1:
                t = base + np.stack([x * rng.integers(1, 6), y * rng.integers(1, 6), (x + y) * rng.integers(1, 4)], -1)
            elif kind == 2:
                t = base + 60.0 * np.sin((x * rng.integers(1, 5) + y * rng.integers(0, 5)) / 2.0)[..., None] * rng.random(3)
            elif kind == 3:
                t = base + rng.normal(0, rng.integers(2, 60), (tile, tile, 3))
            elif kind == 4:
                t = base + rng.normal(0, rng.integers(2, 30), (tile, tile, 1)) * np.ones(3)
            else:
                t = base + 90.0 * np.exp(-((x - tile / 2) ** 2 + (y - tile / 2) ** 2) / rng.integers(8, 200))[..., None] * (rng.random(3) - 0.5)
            out[ty:ty + tile, tx:tx + tile] = np.clip(t, 0, 255).astype(np.uint8)[:h - ty, :w - tx]
    return out


def make_mosaic_pool():
    import numpy as np
    from PIL import Image
    pool = []
    for i in range(64):
        b = io.BytesIO()
        Image.fromarray(mosaic(np.random.default_rng(4321 + i), 640, 480, (16, 32, 64)[i % 3])).save(b, "WEBP", lossless=True)
        pool.append(b.getvalue())
    return pool


def _files(pool):
    folder = tempfile.mkdtemp()
    paths = []
    for i, j in enumerate(pool):
        paths.append(os.path.join(folder, f"{i:03d}.webp"))
        with open(paths[-1], "wb") as f:
            f.write(j)
    return paths


def native(pool, n, route="native", what="(Pillow, lossless=True)"):
    import numpy as np
    import torch

    import bench
    from sds_amd.engine import JpegEngine
    webps = [pool[i % len(pool)] for i in range(n)]
    lens = [len(j) for j in webps]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    blob = torch.from_numpy(np.frombuffer(b"".join(webps), np.uint8).copy()).cuda()
    d_offs, d_lens = torch.from_numpy(offs).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    need = JpegEngine.scratch_need(pool, (256, 256), formats=WEBP) * ((n + len(pool) - 1) // len(pool))
    eng = JpegEngine(max_batch=n, scratch_bytes=need + (64 << 20))
    out, st = eng.decode_resize_device(blob, d_offs, d_lens, (256, 256), formats=WEBP)
    torch.cuda.synchronize()
    assert (st == 0).all(), st[st != 0][:8]
    assert eng.counters()["ok"] == n
    t0 = time.perf_counter()
    for _ in range(3):
        eng.decode_resize_device(blob, d_offs, d_lens, (256, 256), out=out, status=st, formats=WEBP)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    eng.set_timing(True)
    eng.decode_resize_device(blob, d_offs, d_lens, (256, 256), out=out, status=st, formats=WEBP)
    stages = {k: round(v, 3) for k, v in eng.stage_times().items() if v > 0.0005}
    eng.set_timing(False)
    paths = _files(pool)  # the CPU baseline reads files (LoadFromDiskTransform)
    procs = min(16, bench.host_cores())
    cpu1 = bench.cpu_baseline(paths, 1, 2.0)
    cpup = bench.cpu_baseline(paths, procs, 4.0)
    print(json.dumps({"route": route, "metric": f"images/s lossless WebP 640x480 {what} "
                      "decode+resize@256 (device-resident)",
                      "value": round(n / dt, 1), "batch": n, "mean_webp_bytes": round(float(np.mean(lens)), 1),
                      "stage_ms": stages,
                      "cpu_baseline": {"value": round(cpup, 1), "cores": procs, "single_core_value": round(cpu1, 1),
                                       "kind": "reference", "sample": "PIL open+convert, crop, BILINEAR 256x256, "
                                       "CHW tensor over the 64 pool WebPs read from files"}}), flush=True)


def fallback(pool, n):
    import torch

    from sds_amd.batched import GpuDecodeBatch
    from sds_amd.engine import get_engine
    n = min(n, 512)
    webps = [pool[i % len(pool)] for i in range(n)]
    dec = GpuDecodeBatch("webp", (256, 256), device="cuda")
    dec({"webp": webps[:64]})
    torch.cuda.synchronize()
    c0 = get_engine("cuda").counters()
    t0 = time.perf_counter()
    dec({"webp": webps})
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert get_engine("cuda").counters()["fallback"] - c0["fallback"] == n
    print(json.dumps({"route": "fallback", "metric": "images/s lossless WebP 640x480, GpuDecodeBatch default gpu_formats "
                      "(PIL decode per sample in the calling process, resize on the GPU)",
                      "value": round(n / dt, 1), "batch": n}), flush=True)


def latency(pool, n):
    import torch

    from sds_amd.presets import create_standard_image_pipeline
    paths = _files(pool[:16])
    res = {}
    for name, fm in (("native_ms", WEBP), ("default_route_ms", ("jpeg",))):
        ts = create_standard_image_pipeline("webp", (256, 256), device="cuda", service=None, gpu_formats=fm)
        for rep in range(2):  # (the first pass warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p in paths:
                s = {"webp": p}
                for t in ts:
                    s = t(s)
            torch.cuda.synchronize()
            res[name] = round((time.perf_counter() - t0) / len(paths) * 1e3, 3)
    print(json.dumps({"route": "latency", "metric": "ms per one-image call, per-sample transform, lossless WebP 640x480 -> 256x256",
                      **res}), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    routes = sys.argv[2:] or ["native", "fallback", "latency", "mosaic"]
    pool = make_pool()
    for r in routes:
        if r == "mosaic":
            native(make_mosaic_pool(), n, "mosaic", "(Pillow, lossless=True, textured mosaics: tens of prefix-code groups)")
        else:
            {"native": native, "fallback": fallback, "latency": latency}[r](pool, n)


if __name__ == "__main__":
    main()
