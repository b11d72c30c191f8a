"""Throughput of the opt-in native GIF path (k_gif_lzw, k_gif_rgb) next to the routes it replaces: a pool of 64
synthetic 640x480 photos (synth_rgb) written by Pillow as GIF (adaptive 256-colour table), decode + resize to
256x256.  One JSON line per route:

  native     device-resident, formats=("jpeg", "gif")                      (argv[1] images per call)
  fallback   the default route for the same samples: GpuDecodeBatch with gpu_formats=("jpeg",), every GIF
             decoded by PIL in the calling process and resized on the GPU  (at most 512 images)
  latency    one-image calls through the per-sample transform, native and default route (ms per image)

The native line carries the pool's mean file size, bench.cpu_baseline over the pool written to files, on 1 and
16 cores, and the engine's stage times (the two GIF kernels run in the png_inflate slot).
`python tools/gif_bench.py N [route ...]`."""
import io
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GIF = ("jpeg", "gif")


def make_pool():
    import numpy as np
    from PIL import Image

    from tests.golden.synth import synth_rgb
    pool = []
    for i in range(64):
        b = io.BytesIO()
        Image.fromarray(synth_rgb(np.random.default_rng(1234 + i), 640, 480)).save(b, "GIF")
        pool.append(b.getvalue())
    return pool


def _files(pool):
    folder = tempfile.mkdtemp()
    paths = []
    for i, j in enumerate(pool):
        paths.append(os.path.join(folder, f"{i:03d}.gif"))
        with open(paths[-1], "wb") as f:
            f.write(j)
    return paths


def native(pool, n):
    import numpy as np
    import torch

    import bench
    from sds_amd.engine import JpegEngine
    gifs = [pool[i % len(pool)] for i in range(n)]
    lens = [len(j) for j in gifs]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    blob = torch.from_numpy(np.frombuffer(b"".join(gifs), np.uint8).copy()).cuda()
    d_offs, d_lens = torch.from_numpy(offs).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    need = JpegEngine.scratch_need(pool, (256, 256), formats=GIF) * ((n + len(pool) - 1) // len(pool))
    eng = JpegEngine(max_batch=n, scratch_bytes=need + (64 << 20))
    out, st = eng.decode_resize_device(blob, d_offs, d_lens, (256, 256), formats=GIF)
    torch.cuda.synchronize()
    assert (st == 0).all(), st[st != 0][:8]
    assert eng.counters()["ok"] == n
    t0 = time.perf_counter()
    for _ in range(3):
        eng.decode_resize_device(blob, d_offs, d_lens, (256, 256), out=out, status=st, formats=GIF)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    eng.set_timing(True)
    eng.decode_resize_device(blob, d_offs, d_lens, (256, 256), out=out, status=st, formats=GIF)
    stages = {k: round(v, 3) for k, v in eng.stage_times().items() if v > 0.0005}
    eng.set_timing(False)
    paths = _files(pool)  # the CPU baseline reads files (LoadFromDiskTransform)
    procs = min(16, bench.host_cores())
    cpu1 = bench.cpu_baseline(paths, 1, 2.0)
    cpup = bench.cpu_baseline(paths, procs, 4.0)
    print(json.dumps({"route": "native", "metric": "images/s GIF 640x480 (Pillow, adaptive 256-colour table) "
                      "decode+resize@256 (device-resident)",
                      "value": round(n / dt, 1), "batch": n, "mean_gif_bytes": round(float(np.mean(lens)), 1),
                      "stage_ms": stages,
                      "cpu_baseline": {"value": round(cpup, 1), "cores": procs, "single_core_value": round(cpu1, 1),
                                       "kind": "reference", "sample": "PIL open+convert, crop, BILINEAR 256x256, "
                                       "CHW tensor over the 64 pool GIFs read from files"}}), flush=True)


def fallback(pool, n):
    import torch

    from sds_amd.batched import GpuDecodeBatch
    from sds_amd.engine import get_engine
    n = min(n, 512)
    gifs = [pool[i % len(pool)] for i in range(n)]
    dec = GpuDecodeBatch("gif", (256, 256), device="cuda")
    dec({"gif": gifs[:64]})
    torch.cuda.synchronize()
    c0 = get_engine("cuda").counters()
    t0 = time.perf_counter()
    dec({"gif": gifs})
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert get_engine("cuda").counters()["fallback"] - c0["fallback"] == n
    print(json.dumps({"route": "fallback", "metric": "images/s GIF 640x480, GpuDecodeBatch default gpu_formats "
                      "(PIL decode per sample in the calling process, resize on the GPU)",
                      "value": round(n / dt, 1), "batch": n}), flush=True)


def latency(pool, n):
    import torch

    from sds_amd.presets import create_standard_image_pipeline
    paths = _files(pool[:16])
    res = {}
    for name, fm in (("native_ms", GIF), ("default_route_ms", ("jpeg",))):
        ts = create_standard_image_pipeline("gif", (256, 256), device="cuda", service=None, gpu_formats=fm)
        for rep in range(2):  # (the first pass warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p in paths:
                s = {"gif": p}
                for t in ts:
                    s = t(s)
            torch.cuda.synchronize()
            res[name] = round((time.perf_counter() - t0) / len(paths) * 1e3, 3)
    print(json.dumps({"route": "latency", "metric": "ms per one-image call, per-sample transform, GIF 640x480 -> 256x256",
                      **res}), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    routes = sys.argv[2:] or ["native", "fallback", "latency"]
    pool = make_pool()
    for r in routes:
        {"native": native, "fallback": fallback, "latency": latency}[r](pool, n)


if __name__ == "__main__":
    main()
