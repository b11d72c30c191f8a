"""What the GPU tests of the opt-in PNG masks (test_gpu_png.py, test_gpu_png_ext.py, test_gpu_png_meta.py) share:
the native-decode check of a group, the blob packing of the device-resident entry point, and the comparison of the
opt-in route with the default route on damaged and handed-over files.  Each test file keeps its own fixtures, masks,
sample lists and parametrised tests."""
import os
import tempfile

import numpy as np
import torch

from tests import png_synth as S
from tests.test_gpu_frames import _ref


def by_size(cases):
    out = {}
    for n, d, ref in cases:
        out.setdefault(ref.shape[:2], []).append((n, d, ref))
    return out


def decode_group_natively(engine, cases, formats):
    """The group through GpuDecodeBatch(gpu_formats=formats) at each image's own size (the decode alone): pixels
    equal PIL's, every sample counted as native PNG, none as a PIL fallback."""
    from sds_amd.batched import GpuDecodeBatch
    c0 = engine.counters()
    total = 0
    for (h, w), group in by_size(cases).items():
        batch = GpuDecodeBatch("png", (h, w), device="cuda", gpu_formats=formats, on_error="raise")(
            {"png": [d for _, d, _ in group], "name": [n for n, _, _ in group]})
        img = batch["image"].cpu().numpy()
        assert img.shape == (len(group), 3, h, w)
        for k, (n, _, ref) in enumerate(group):
            np.testing.assert_array_equal(img[k], ref.transpose(2, 0, 1), err_msg=n)
        total += len(group)
    c1 = engine.counters()
    assert c1["png"] - c0["png"] == total
    assert c1["fallback"] - c0["fallback"] == 0
    assert c1["ok"] - c0["ok"] == total


def pack_device(samples):
    """(blob, offsets, lengths) on the device, every sample at a multiple of 16 bytes."""
    lens = np.array([len(s) for s in samples], np.int32)
    offs = np.concatenate([[0], np.cumsum((lens.astype(np.int64) + 15) // 16 * 16)[:-1]]).astype(np.int64)
    blob = np.zeros(int(offs[-1] + lens[-1] + 16), np.uint8)
    for s, o in zip(samples, offs):
        blob[o:o + len(s)] = np.frombuffer(s, np.uint8)
    return torch.from_numpy(blob).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda()


def decode_device(engine, samples, res, formats, flip=None, **kw):
    """The device-resident entry point on host bytes: (output, statuses)."""
    from sds_amd.engine import JpegEngine
    engine.reserve(JpegEngine.scratch_need(samples, res, formats=formats, **kw))
    if flip is not None:
        kw["flip"] = torch.tensor(flip, dtype=torch.uint8).cuda()
    out, st = engine.decode_resize_device(*pack_device(samples), res, formats=formats, **kw)
    return out.cpu().numpy(), st.cpu().numpy()


def assert_rows_equal(outs, ref):
    """Every entry point of outs (name -> (output, statuses)) decoded every sample, to ref's rows."""
    for name, (o, st) in outs.items():
        assert (st == 0).all(), (name, st)
        for k in range(len(ref)):
            np.testing.assert_array_equal(o[k], ref[k], err_msg=f"{name} row {k}")


def run_transforms(transforms, sample):
    for t in transforms:
        sample = t(sample)
    return sample


def pipeline_outcome(path, **kw):
    from sds_amd.presets import create_standard_image_pipeline
    try:
        s = run_transforms(create_standard_image_pipeline("png", (16, 20), device="cuda", service=None, **kw), {"png": path})
        return "ok", s["image"].cpu().contiguous().numpy()
    except Exception as e:  # noqa: BLE001 -- the exception type is what is compared
        return "err", type(e)


def check_handover_and_damage(engine, data, formats, good):
    """The opt-in route (mask `formats`) gives the same tensor or the same exception type as the default route on
    `data`: through the per-sample pipeline, in a batch between two `good` samples, and at engine level."""
    from sds_amd.batched import GpuDecodeBatch
    p = os.path.join(tempfile.mkdtemp(), "x.png")
    with open(p, "wb") as f:
        f.write(data)
    a, b = pipeline_outcome(p, gpu_formats=formats), pipeline_outcome(p)
    assert a[0] == b[0], (a, b)
    if a[0] == "ok":
        np.testing.assert_array_equal(a[1], b[1])
    else:
        assert a[1] is b[1]
    outs = []
    for fm in (formats, ("jpeg",)):
        try:
            r = GpuDecodeBatch("png", (16, 20), device="cuda", gpu_formats=fm, on_error="raise")({"png": [good, data, good]})
            outs.append(("ok", r["image"].cpu().numpy()))
        except Exception as e:  # noqa: BLE001
            outs.append(("err", type(e)))
    assert outs[0][0] == outs[1][0] == a[0]
    if outs[0][0] == "ok":
        np.testing.assert_array_equal(outs[0][1], outs[1][1])
    else:
        assert outs[0][1] is outs[1][1]
    # engine level: status 0 only where PIL decodes the same bytes, and then to the same pixels
    kind, ref = S.pil_outcome(data)
    out, st = engine.decode_resize([data], (16, 20), formats=formats)
    if kind == "err":
        assert st[0] != 0
    if st[0] == 0:
        assert kind == "ok"
        np.testing.assert_array_equal(out[0].cpu().numpy(), _ref(ref, (16, 20)))
