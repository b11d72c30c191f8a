"""The opt-in "jpeg-ext" mask on the host (no GPU): the bit's value and names, mask validity, the status of every
fixture of tests/jpeg_ext_synth.py under the default mask and under the bit (sdsj_plan_need_formats,
sdsj_probe_formats), and the planner under the mask in a stand-alone ASan + UBSan program
(tests/asan/jpeg_ext_driver.cpp, its own main; nothing sanitized is loaded into Python).

Every ext fixture decodes on PIL; the refused cases (a fractional ratio, 16 blocks per MCU, CMYK) are refused under
either mask."""
import ctypes
import shutil

import pytest

from sds_amd import _lib as L
from tests import asan_harness as H
from tests import jpeg_ext_synth as J

EXT = L.FORMAT_JPEG | 64


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _need(lib, data, mask, crop=1):
    op = L.SdsjOp(16, 20, crop, L.FILTERS["bilinear"], L.DTYPE_U8, L.LAYOUT_CHW)
    need = ctypes.c_int64(-1)
    st = lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need))
    return st, need.value


def test_values_and_names():
    assert L.FORMAT_JPEG_EXT == 64
    assert L.FORMATS["jpeg-ext"] == 65
    assert L.format_mask(("jpeg", "jpeg-ext")) == 65
    assert L.format_mask(("jpeg-ext", "png-meta")) == 83
    assert "sdsj_probe_formats" in L.EXPORTS


def test_mask_validity(lib):
    data = J.ext_fixtures()[0][1]
    for mask in (64, 66, 8, 15, 32, 51):
        assert _need(lib, data, mask)[0] == L.EINVAL, mask
    for mask in (65, 67, 87):
        assert _need(lib, data, mask)[0] == L.OK, mask
    info = L.SdsjInfo()
    assert lib.sdsj_probe_formats(data, len(data), 64, ctypes.byref(info)) == L.EINVAL


def test_status_of_every_fixture(lib):
    fx = J.ext_fixtures()
    assert len(fx) == len(J.SETS) * len(J.SIZES) + 1 + 4 + 4 + 7
    for name, data in fx:
        ref = J.pil_rgb(data)  # (PIL decodes every ext fixture)
        assert _need(lib, data, L.FORMAT_JPEG) == (L.UNSUPPORTED, 0), name
        st, need = _need(lib, data, EXT)
        assert st == L.OK and need > 0, (name, st, need)
        st, info = L.probe(data, EXT)
        assert st == L.OK and info.supported == 1, name
        assert (info.height, info.width) == ref.shape[:2], name
        st, info = L.probe(data)  # sdsj_probe answers as before
        assert st == L.UNSUPPORTED and info.supported == 0, name
        assert (info.height, info.width) == ref.shape[:2], name


def test_jfif_wins_over_adobe_transform_0(lib):
    data = J.jfif_and_adobe0()
    a, b = _need(lib, data, L.FORMAT_JPEG), _need(lib, data, EXT)
    assert a[0] == L.OK and a == b
    assert L.probe(data)[0] == L.OK and L.probe(data, EXT)[0] == L.OK


def test_refused_under_either_mask(lib):
    for name, data in J.refused():
        for mask in (L.FORMAT_JPEG, EXT):
            st, need = _need(lib, data, mask)
            assert st in (L.UNSUPPORTED, L.CORRUPT) and need == 0, (name, mask, st)
            assert L.probe(data, mask)[0] == st, (name, mask)
    for name in ("fractional", "luma4x4"):  # (Pillow refuses these too)
        assert J.pil_outcome(dict(J.refused())[name])[0] == "err", name


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_planner_under_the_mask_under_asan_and_ubsan():
    whole = [d for _, d in J.ext_fixtures()] + [J.jfif_and_adobe0()] + [d for _, d in J.refused()] + \
        [d for _, d in J.damaged()]
    # header damage on one file of every kind (the truncations of all 52 would only repeat the same headers)
    picks = dict(J.ext_fixtures())
    seeds = [picks[k] for k in ("411-50x37", "2x4-33x70", "cr42-5x9", "mixed-50x37-dri3", "mixed-50x37-prog",
                                "rgb-pillow", "rgb-pillow-prog", "rgb-adobe0-411", "rgb-ids-411-dri")]
    inputs = whole + J.header_mutations(seeds)
    exe = H.build("jpeg_ext_driver.cpp", "address,undefined", ("-I", H.INCLUDE))
    rows = H.run_records(exe, inputs, H.ASAN_UBSAN)
    n_ext = len(J.ext_fixtures())
    for (name, _), row in zip(J.ext_fixtures(), rows[:n_ext]):
        st, need, fused, rr, unfused, is_ext = row[:6]
        assert st == 0 and need > 0 and is_ext == 1 and fused == 0 and rr == unfused, (name, row)
    seen_ok = 0
    for row in rows:  # every OK ext image, damaged headers included, takes the unfused passes
        if row[0] == 0 and row[5] == 1:
            assert row[2] == 0 and row[3] == row[4], row
            seen_ok += 1
    assert seen_ok > n_ext
    try:
        lib = L.load()
    except Exception:  # noqa: BLE001  (the product library is not built: the sanitized run is the check)
        return
    for x, row in zip(inputs, rows):
        st, need = _need(lib, x, EXT, crop=0)  # (the driver's op)
        assert (st, need) == (row[0], row[1]), (len(x), st, need, row)
