"""Throughput of the opt-in native PNG path (k_png_inflate, k_png_unfilter) next to the routes it replaces:
a pool of 64 synthetic 640x480 RGB PNGs (synth_rgb, Pillow's default compression), decode + resize to
256x256.  One JSON line per route:

  native     device-resident, formats=("jpeg", "png")                      (argv[1] images per call)
  fallback   the default route for the same samples: GpuDecodeBatch with gpu_formats=("jpeg",), every PNG
             decoded by PIL in the calling process and resized on the GPU  (at most 512 images)
  latency    one-image calls through the per-sample transform, native and default route (ms per image)

The native line carries bench.cpu_baseline over the pool written to files, on 1 and 16 cores, and the
engine's stage times (png_inflate / png_unfilter among them).  `python tools/png_bench.py N [route ...]`.

`--ext` measures the wider subset instead (formats=("jpeg", "png-ext"), k_png_unfilter_ext): the same 64
images as Adam7-interlaced RGB (written by tests/png_ext_synth.py, Pillow writes no interlaced files) and as
4-bit palette files (Pillow's quantize to 16 colours, bits=4), after the base pool itself under the full mask;
every line then carries a "case".

`--meta` measures files as editors write them (formats=("jpeg", "png-meta"), k_png_meta): the base pool re-saved
through Pillow with an ICC profile of about 3 KB (arbitrary bytes: Pillow does not parse them), a compressed iTXt
XMP-like packet of about 4 KB and a tEXt appended after the image data, after the base pool itself under that
mask; the "parse" stage holds k_parse (now with the CRC of the profile) and k_png_meta."""
import io
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BOTH = ("jpeg", "png")
EXT = ("jpeg", "png-ext")
META = ("jpeg", "png-meta")


def make_pool():
    import numpy as np
    from PIL import Image

    from tests.golden.synth import synth_rgb
    pool = []
    for i in range(64):
        b = io.BytesIO()
        Image.fromarray(synth_rgb(np.random.default_rng(1234 + i), 640, 480)).save(b, "PNG")
        pool.append(b.getvalue())
    return pool


def make_ext_pools():
    import numpy as np
    from PIL import Image

    from tests import png_ext_synth as E
    from tests import png_synth as S
    from tests.golden.synth import synth_rgb
    adam7, pal4 = [], []
    for i in range(64):
        rgb = synth_rgb(np.random.default_rng(1234 + i), 640, 480)
        raw = E.raw_stream(rgb.astype(np.uint16), 2, 8, 1, "all4")
        adam7.append(S.write_png(640, 480, 2, S.zstream(raw, 6), interlace=1))
        b = io.BytesIO()
        Image.fromarray(rgb).quantize(16).save(b, "PNG", bits=4)
        pal4.append(b.getvalue())
    return [("adam7 RGB", adam7), ("4-bit palette", pal4)]


def make_meta_pool():
    import numpy as np
    from PIL import Image
    from PIL.PngImagePlugin import PngInfo

    from tests import png_synth as S
    from tests.golden.synth import synth_rgb
    pool = []
    for i in range(64):
        rng = np.random.default_rng(1234 + i)
        rgb = synth_rgb(rng, 640, 480)
        info = PngInfo()
        info.add_itxt("XML:com.adobe.xmp", "<x:xmpmeta>" + "".join(f"<rdf:li>{int(v)}</rdf:li>" for v in rng.integers(0, 1 << 30, 200))
                      + "</x:xmpmeta>", zip=True)
        b = io.BytesIO()
        Image.fromarray(rgb).save(b, "PNG", icc_profile=rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), pnginfo=info)
        data = b.getvalue()
        k = data.rindex(b"IEND") - 4
        pool.append(data[:k] + S.chunk(b"tEXt", b"Comment\0written after the image data") + data[k:])
    return pool


def native(pool, n, formats=BOTH, case=None):
    import numpy as np
    import torch

    import bench
    from sds_amd.engine import JpegEngine
    pngs = [pool[i % len(pool)] for i in range(n)]
    lens = [len(j) for j in pngs]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    blob = torch.from_numpy(np.frombuffer(b"".join(pngs), np.uint8).copy()).cuda()
    d_offs, d_lens = torch.from_numpy(offs).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    need = JpegEngine.scratch_need(pool, (256, 256), formats=formats) * ((n + len(pool) - 1) // len(pool))
    eng = JpegEngine(max_batch=n, scratch_bytes=need + (64 << 20))
    out, st = eng.decode_resize_device(blob, d_offs, d_lens, (256, 256), formats=formats)
    torch.cuda.synchronize()
    assert (st == 0).all(), st[st != 0][:8]
    assert eng.counters()["png"] == n
    t0 = time.perf_counter()
    for _ in range(3):
        eng.decode_resize_device(blob, d_offs, d_lens, (256, 256), out=out, status=st, formats=formats)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    eng.set_timing(True)
    eng.decode_resize_device(blob, d_offs, d_lens, (256, 256), out=out, status=st, formats=formats)
    stages = {k: round(v, 3) for k, v in eng.stage_times().items() if v > 0.0005}
    eng.set_timing(False)
    folder = tempfile.mkdtemp()
    paths = []
    for i, j in enumerate(pool):  # the CPU baseline reads files (LoadFromDiskTransform)
        paths.append(os.path.join(folder, f"{i:03d}.png"))
        with open(paths[-1], "wb") as f:
            f.write(j)
    procs = min(16, bench.host_cores())
    cpu1 = bench.cpu_baseline(paths, 1, 2.0)
    cpup = bench.cpu_baseline(paths, procs, 4.0)
    print(json.dumps({"route": "native", **({"case": case} if case else {}),
                      "metric": f"images/s PNG 640x480 {case or 'RGB'} decode+resize@256 (device-resident)",
                      "value": round(n / dt, 1), "batch": n, "mean_png_bytes": round(float(np.mean(lens)), 1),
                      "stage_ms": stages,
                      "cpu_baseline": {"value": round(cpup, 1), "cores": procs, "single_core_value": round(cpu1, 1),
                                       "kind": "reference", "sample": "PIL open+convert, crop, BILINEAR 256x256, "
                                       "CHW tensor over the 64 pool PNGs read from files"}}), flush=True)


def fallback(pool, n, formats=BOTH, case=None):
    import torch

    from sds_amd.batched import GpuDecodeBatch
    from sds_amd.engine import get_engine
    n = min(n, 512)
    pngs = [pool[i % len(pool)] for i in range(n)]
    dec = GpuDecodeBatch("png", (256, 256), device="cuda")
    dec({"png": pngs[:64]})
    torch.cuda.synchronize()
    c0 = get_engine("cuda").counters()
    t0 = time.perf_counter()
    dec({"png": pngs})
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert get_engine("cuda").counters()["fallback"] - c0["fallback"] == n
    print(json.dumps({"route": "fallback", **({"case": case} if case else {}),
                      "metric": f"images/s PNG 640x480 {case or 'RGB'}, GpuDecodeBatch default gpu_formats "
                      "(PIL decode per sample in the calling process, resize on the GPU)",
                      "value": round(n / dt, 1), "batch": n}), flush=True)


def latency(pool, n, formats=BOTH, case=None):
    import torch

    from sds_amd.presets import create_standard_image_pipeline
    folder = tempfile.mkdtemp()
    paths = []
    for i, j in enumerate(pool[:16]):
        paths.append(os.path.join(folder, f"{i:03d}.png"))
        with open(paths[-1], "wb") as f:
            f.write(j)
    res = {}
    for name, fm in (("native_ms", formats), ("default_route_ms", ("jpeg",))):
        ts = create_standard_image_pipeline("png", (256, 256), device="cuda", service=None, gpu_formats=fm)
        for rep in range(2):  # (the first pass warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p in paths:
                s = {"png": p}
                for t in ts:
                    s = t(s)
            torch.cuda.synchronize()
            res[name] = round((time.perf_counter() - t0) / len(paths) * 1e3, 3)
    print(json.dumps({"route": "latency", **({"case": case} if case else {}),
                      "metric": f"ms per one-image call, per-sample transform, PNG 640x480 {case or 'RGB'} -> 256x256",
                      **res}), flush=True)


def main():
    args = [a for a in sys.argv[1:] if a not in ("--ext", "--meta")]
    ext, meta = "--ext" in sys.argv[1:], "--meta" in sys.argv[1:]
    n = int(args[0]) if args else 4096
    routes = args[1:] or ["native", "fallback", "latency"]
    # (--ext: the base pool too, so that what the full mask costs plain 8-bit files is on record)
    if meta:
        pools = [("RGB under png-meta", make_pool()), ("RGB with iCCP, iTXt and a trailing tEXt", make_meta_pool())]
    else:
        pools = [("RGB under png-ext", make_pool())] + make_ext_pools() if ext else [(None, make_pool())]
    for case, pool in pools:
        for r in routes:
            {"native": native, "fallback": fallback, "latency": latency}[r](pool, n, META if meta else EXT if ext else BOTH, case)


if __name__ == "__main__":
    main()
