"""The opt-in "jpeg-cmyk-prog" mask on the host (no GPU): the bit's value and names, mask validity on
sdsj_plan_need_formats and sdsj_probe_formats, the status of every fixture of tests/jpeg_cmyk_prog_synth.py under its own
mask, under the full one and under the masks that lack the bit, PIL's outcome class of every fixture, and the parser and
planner under the new masks in a stand-alone ASan + UBSan program (tests/asan/jpeg_cmyk_prog_driver.cpp, its own main;
nothing sanitized is loaded into Python)."""
import ctypes
import shutil

import numpy as np
import pytest

from sds_amd import _lib as L
from tests import asan_harness as H
from tests import jpeg_cmyk_prog_synth as PS
from tests import jpeg_cmyk_synth as S
from tests import jpeg_ext_synth as J

FULL = 1537 + 64 + 128
WITHOUT = (1, 65, 129, 193, 513, 577, 641, 705)  # every JPEG mask that lacks the bit


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _need(lib, data, mask, crop=1):
    op = L.SdsjOp(16, 20, crop, L.FILTERS["bilinear"], L.DTYPE_U8, L.LAYOUT_CHW)
    need = ctypes.c_int64(-1)
    st = lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need))
    return st, need.value


def test_values_and_names():
    assert L.FORMAT_JPEG_CMYK_PROG == 1024
    assert L.FORMATS["jpeg-cmyk-prog"] == 1537
    assert L.format_mask(("jpeg-cmyk-prog",)) == 1537
    assert L.format_mask(("jpeg", "jpeg-cmyk", "jpeg-cmyk-prog")) == 1537
    assert L.format_mask(("jpeg-cmyk-prog", "jpeg-ext")) == 1537 + 64
    assert L.format_mask(("jpeg-cmyk-prog", "jpeg-scans")) == 1537 + 128
    assert L.format_mask(("jpeg-cmyk-prog", "gif")) == 1537 + 256
    assert L.format_mask(("jpeg-cmyk-prog", "png", "png-ext", "png-meta")) == 1537 + 2 + 4 + 16
    assert L.format_mask(PS.PROG) == 1537 and L.format_mask(PS.PROG_EXT) == 1601 and L.format_mask(PS.MIXED) == FULL
    assert L.format_mask(("jpeg-cmyk",)) == 513  # (the older name does not carry the new bit)


VALID = (1537, 1537 + 64, 1537 + 128, FULL, 1537 + 2, 1537 + 256, 1537 + 2 + 4 + 16, 2047 - 8 - 32)
INVALID = (1024, 1025, 1536, 1024 + 2, 1024 + 256, 1024 + 64 + 1, 1024 + 128 + 1, 1024 + 512 + 2, 1537 + 8, 1537 + 32, 2048,
           2048 + 1537)


def test_mask_validity(lib):
    data = PS.clean()[0][1]
    info = L.SdsjInfo()
    for mask in INVALID:
        assert _need(lib, data, mask)[0] == L.EINVAL, mask
    for mask in (1024, 1025, 1536):
        assert lib.sdsj_probe_formats(data, len(data), mask, ctypes.byref(info)) == L.EINVAL, mask
    for mask in VALID:
        assert _need(lib, data, mask)[0] == L.OK, mask
    for mask in (1537, 1537 + 64, 1537 + 128, FULL):
        assert lib.sdsj_probe_formats(data, len(data), mask, ctypes.byref(info)) == L.OK and info.supported == 1, mask


def test_status_of_every_clean_and_cut_fixture(lib):
    """OK under the file's own mask and the full one, with equal needs; refused with need == 0 under every mask that
    lacks the bit (UNSUPPORTED at the frame header), and under "jpeg-cmyk-prog" alone when it needs "jpeg-ext" too.  A
    file cut in the middle of a scan has whole headers: what is wrong with it is the device's to find."""
    fx = PS.clean() + PS.end_cuts() + PS.mid_cuts_eoi() + PS.mid_cuts()
    assert len(PS.clean()) == PS.N_CLEAN == 32 and len(fx) == 32 + 34 + 4 + 4
    for name, data, formats, _ in fx:
        own = L.format_mask(formats)
        size = _size(data)
        for mask in WITHOUT:
            assert _need(lib, data, mask) == (L.UNSUPPORTED, 0), (name, mask)
            st, info = L.probe(data, mask)
            assert st == L.UNSUPPORTED and info.supported == 0, (name, mask)
        st, info = L.probe(data)  # sdsj_probe answers as before
        assert st == L.UNSUPPORTED and info.supported == 0, name
        for mask in (1537, own, FULL):
            want = L.OK if mask & own == own else L.UNSUPPORTED
            st, need = _need(lib, data, mask)
            assert st == want and (need > 0) == (want == L.OK), (name, mask, st, need)
            st, info = L.probe(data, mask)
            assert st == want and info.supported == (want == L.OK), (name, mask)
            assert (info.width, info.height) == size and info.ncomp == 4, name
        assert _need(lib, data, own) == _need(lib, data, FULL), name


def _size(data):
    p = data.index(b"\xff\xc2")
    return int.from_bytes(data[p + 7:p + 9], "big"), int.from_bytes(data[p + 5:p + 7], "big")


def test_refused_statuses(lib):
    by_name = {n: d for n, d, _, _ in PS.refused()}
    assert sorted(by_name) == ["fractional", "sixteen-blocks"]
    for name, data in by_name.items():
        for mask in WITHOUT:
            assert _need(lib, data, mask) == (L.UNSUPPORTED, 0), (name, mask)
        want = L.CORRUPT if name == "sixteen-blocks" else L.UNSUPPORTED
        for mask in (1537, 1601, 1665, FULL):
            assert _need(lib, data, mask) == (want, 0), (name, mask)
            st, info = L.probe(data, mask)
            assert st == want and info.supported == 0, (name, mask)


def test_sequential_files_plan_alike_with_and_without_the_bit(lib):
    """What "jpeg-cmyk" decodes keeps its status and its need under "jpeg-cmyk-prog"; the file the older tests pin as
    refused under 513 .. 705 is the one the bit admits."""
    for name, data, formats, _ in S.fixtures():
        own = L.format_mask(formats)
        assert _need(lib, data, own) == _need(lib, data, own | 1024), name
    name, data, _, _ = S.refused()[0]
    assert name == "progressive-pillow"
    for mask in (513, 577, 641, 705):
        assert _need(lib, data, mask) == (L.UNSUPPORTED, 0)
        st, need = _need(lib, data, mask | 1024)
        assert st == L.OK and need > 0


def test_every_fixture_has_the_pil_outcome_its_class_claims():
    """No case can drop out silently: every file listed "ok" decodes in this PIL, every "err" one raises OSError."""
    classes = []
    for name, data, _, cls in PS.fixtures():
        kind, what = J.pil_outcome(data)
        assert kind == cls and (kind == "ok" or what is OSError), (name, kind, what)
        classes.append(cls)
    assert classes == ["ok"] * (32 + 34 + 4) + ["err"] * (4 + 2)
    # what Pillow writes is what the fixtures' description says: 18 scans, the DC ones over all four components
    for src in PS.CUT_SOURCES:
        data = PS._pil(src)
        spans = PS.scan_spans(data)
        assert len(spans) == 18 and [data[s + 4] for s, _, _ in spans] == [4] + [1] * 12 + [4] + [1] * 4
    # a YCCK twin differs from its CMYK source in PIL (the transform byte is what chooses the colour space)
    assert not np.array_equal(J.pil_rgb(PS._pil("pil-ss0-q95-17x23")), J.pil_rgb(dict((n, d) for n, d, _, _ in PS.ycck_files())["ycck2-ss0-17x23"]))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_parser_and_planner_under_the_masks_under_asan_and_ubsan():
    fx = PS.fixtures()
    whole = [d for _, d, _, _ in fx]
    small = min((d for _, d, _, _ in PS.pillow_files()), key=len)  # the smallest Pillow file: every byte cut, and damage in its headers
    assert _size(small) == (1, 1)
    cuts = [small[:k] for k in range(len(small))]
    first = small.index(b"\xff\xda")
    rng = np.random.default_rng(7)
    damage = []
    for k in range(first + 14):  # every header byte up to the end of the first SOS, one value each
        b = bytearray(small)
        b[k] = int(rng.choice([0xFF, 0x00, 0xC2, 0xC0, 0xDA, 0xD9, 0x04, 0x11, 0x22, 0x41, int(rng.integers(0, 256))]))
        damage.append(bytes(b))
    inputs = whole + cuts + damage
    exe = H.build("jpeg_cmyk_prog_driver.cpp", "address,undefined", ("-I", H.INCLUDE))
    rows = H.run_records(exe, inputs, H.ASAN_UBSAN)
    assert len(rows) == len(inputs)
    masks = (1537, 1601, 1665, FULL)
    ok_classes = len(PS.clean()) + len(PS.end_cuts()) + len(PS.mid_cuts_eoi()) + len(PS.mid_cuts())
    for k, ((name, _, formats, _), row) in enumerate(zip(fx, rows)):
        own = L.format_mask(formats)
        rt_prog4, rt_scans, ncomp = row[16:19]
        assert ncomp == 4 and rt_prog4 != rt_scans, (name, row)
        for q, mask in enumerate(masks):
            st, need, prog, re = row[4 * q:4 * q + 4]
            if k >= ok_classes:
                assert st in (L.UNSUPPORTED, L.CORRUPT) and need == 0, (name, mask, row)
            elif mask & own == own:  # a route of its own, SOF2's progressive == 1
                assert st == 0 and need > 0 and prog == 1 and re == rt_prog4, (name, mask, row)
            else:
                assert st == L.UNSUPPORTED and need == 0, (name, mask, row)
    for row in rows:  # whatever the bytes: an accepted progressive file of four components takes the new route, and
        for q in range(4):  # nothing else does
            if row[4 * q] == 0 and row[4 * q + 1] > 0:
                assert (row[4 * q + 3] == row[16]) == (row[4 * q + 2] == 1 and row[18] == 4), row
    try:
        lib = L.load()
    except Exception:  # noqa: BLE001  (the product library is not built: the sanitized run is the check)
        return
    for x, row in zip(inputs, rows):
        for q, mask in enumerate(masks):
            st, need = _need(lib, x, mask, crop=0)  # (the driver's op and masks)
            assert (st, need) == (row[4 * q], row[4 * q + 1]), (len(x), mask, st, need, row)
