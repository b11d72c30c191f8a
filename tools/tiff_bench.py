"""Throughput of the opt-in native TIFF path (k_tiff_copy, k_tiff_lzw, k_tiff_inflate, k_tiff_rgb) next to the routes
it replaces: pools of 64 synthetic 640x480 photos (synth_rgb, the pixels of tools/png_bench.py's pool) written by
Pillow as TIFF with compression "tiff_lzw", "tiff_adobe_deflate", "packbits" and "raw" (uncompressed), decode + resize
to 256x256.  Pillow / libtiff write the compressed files in strips of about 64 KiB (15 strips of 34 rows for RGB);
Pillow writes an uncompressed file as one strip, which the sample's wavefronts of k_tiff_copy share: that pool shows
the cost of the copy alone.  One JSON line per route and pool:

  native     device-resident, formats=("jpeg", "tiff")                     (argv[1] images per call)
  fallback   the default route for the same samples: GpuDecodeBatch with gpu_formats=("jpeg",), every TIFF
             decoded by PIL in the calling process and resized on the GPU  (at most 512 images)
  latency    one-image calls through the per-sample transform, native and default route (ms per image)

The native line carries the pool's mean file size and strip count, bench.cpu_baseline over the pool written to
files, on 1 and 16 cores, and the engine's stage times (the TIFF kernels run in the png_inflate slot).  The stage times
are event intervals summed over the call's lanes, which run on two streams: while one lane's inflate kernel fills the
register files, the other lane's short kernels (parse, plan, ...) wait, and the wait counts in their intervals.
`python tools/tiff_bench.py N [route ...] [--comp NAME ...]`."""
import io
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TIFF = ("jpeg", "tiff")
COMPS = ("tiff_lzw", "tiff_adobe_deflate", "packbits", "raw")


def make_pool(comp):
    import numpy as np
    from PIL import Image

    from tests.golden.synth import synth_rgb
    pool = []
    for i in range(64):
        b = io.BytesIO()
        Image.fromarray(synth_rgb(np.random.default_rng(1234 + i), 640, 480)).save(b, "TIFF", compression=comp)
        pool.append(b.getvalue())
    return pool


def _files(pool):
    folder = tempfile.mkdtemp()
    paths = []
    for i, j in enumerate(pool):
        paths.append(os.path.join(folder, f"{i:03d}.tif"))
        with open(paths[-1], "wb") as f:
            f.write(j)
    return paths


def native(pool, n, comp):
    import numpy as np
    import torch

    import bench
    from sds_amd import _lib
    from sds_amd.engine import JpegEngine
    tiffs = [pool[i % len(pool)] for i in range(n)]
    lens = [len(j) for j in tiffs]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    blob = torch.from_numpy(np.frombuffer(b"".join(tiffs), np.uint8).copy()).cuda()
    d_offs, d_lens = torch.from_numpy(offs).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    need = JpegEngine.scratch_need(pool, (256, 256), formats=TIFF) * ((n + len(pool) - 1) // len(pool))
    eng = JpegEngine(max_batch=n, scratch_bytes=need + (64 << 20))
    out, st = eng.decode_resize_device(blob, d_offs, d_lens, (256, 256), formats=TIFF)
    torch.cuda.synchronize()
    assert (st == 0).all(), st[st != 0][:8]
    assert eng.counters()["ok"] == n
    t0 = time.perf_counter()
    for _ in range(3):
        eng.decode_resize_device(blob, d_offs, d_lens, (256, 256), out=out, status=st, formats=TIFF)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    eng.set_timing(True)
    eng.decode_resize_device(blob, d_offs, d_lens, (256, 256), out=out, status=st, formats=TIFF)
    stages = {k: round(v, 3) for k, v in eng.stage_times().items() if v > 0.0005}
    eng.set_timing(False)
    paths = _files(pool)  # the CPU baseline reads files (LoadFromDiskTransform)
    procs = min(16, bench.host_cores())
    cpu1 = bench.cpu_baseline(paths, 1, 2.0)
    cpup = bench.cpu_baseline(paths, procs, 4.0)
    print(json.dumps({"route": "native", "compression": comp,
                      "metric": f"images/s TIFF 640x480 RGB (Pillow, compression={comp}) decode+resize@256 (device-resident)",
                      "value": round(n / dt, 1), "batch": n, "mean_tiff_bytes": round(float(np.mean(lens)), 1),
                      "strips": int(_lib.tiff_probe(pool[0])[1].strips), "stage_ms": stages,
                      "cpu_baseline": {"value": round(cpup, 1), "cores": procs, "single_core_value": round(cpu1, 1),
                                       "kind": "reference", "sample": "PIL open+convert, crop, BILINEAR 256x256, "
                                       "CHW tensor over the 64 pool TIFFs read from files"}}), flush=True)


def fallback(pool, n, comp):
    import torch

    from sds_amd.batched import GpuDecodeBatch
    from sds_amd.engine import get_engine
    n = min(n, 512)
    tiffs = [pool[i % len(pool)] for i in range(n)]
    dec = GpuDecodeBatch("tiff", (256, 256), device="cuda")
    dec({"tiff": tiffs[:64]})
    torch.cuda.synchronize()
    c0 = get_engine("cuda").counters()
    t0 = time.perf_counter()
    dec({"tiff": tiffs})
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert get_engine("cuda").counters()["fallback"] - c0["fallback"] == n
    print(json.dumps({"route": "fallback", "compression": comp,
                      "metric": f"images/s TIFF 640x480 RGB (compression={comp}), GpuDecodeBatch default gpu_formats "
                      "(PIL decode per sample in the calling process, resize on the GPU)",
                      "value": round(n / dt, 1), "batch": n}), flush=True)


def latency(pool, n, comp):
    import torch

    from sds_amd.presets import create_standard_image_pipeline
    paths = _files(pool[:16])
    res = {}
    for name, fm in (("native_ms", TIFF), ("default_route_ms", ("jpeg",))):
        ts = create_standard_image_pipeline("tiff", (256, 256), device="cuda", service=None, gpu_formats=fm)
        for rep in range(2):  # (the first pass warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p in paths:
                s = {"tiff": p}
                for t in ts:
                    s = t(s)
            torch.cuda.synchronize()
            res[name] = round((time.perf_counter() - t0) / len(paths) * 1e3, 3)
    print(json.dumps({"route": "latency", "compression": comp,
                      "metric": f"ms per one-image call, per-sample transform, TIFF 640x480 RGB (compression={comp}) -> 256x256",
                      **res}), flush=True)


def main():
    args, comps = [], []
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--comp":
            comps.append(next(it))
        else:
            args.append(a)
    n = int(args[0]) if args else 4096
    routes = args[1:] or ["native", "fallback", "latency"]
    for comp in comps or COMPS:
        pool = make_pool(comp)
        for r in routes:
            {"native": native, "fallback": fallback, "latency": latency}[r](pool, n, comp)


if __name__ == "__main__":
    main()
