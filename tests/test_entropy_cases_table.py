"""The entropy / unstuff case table (tests/entropy_cases.py), proved on the CPU: the real plan_sample
(tests/asan/plan_driver.cpp, stand-alone and sanitized, built as tests/test_plan_host.py builds it) plans every
case in both modes, and every situation a case pins holds for its plan; the table holds every situation, so one
that loses a situation fails here, without a GPU.  The byte-level properties -- the straddled pairs, the fill
padding, the scan's start residues -- are checked by scanning the bytes.

``unstuff`` is a short restatement of the unstuffing and restart split (jdhuff.c jpeg_fill_bit_buffer /
process_restart for a well-formed file), checked against PIL: a file re-assembled from its segments decodes to
the original's pixels.  It is the stage reference of tests/test_gpu_entropy_routes.py, which also imports
``plan_table``: the plan driver's fields per (case, mode), so the formulas are restated nowhere."""
import io
import os

import numpy as np
import pytest

from tests import entropy_cases as E
from tests import test_plan_host as H
from tests.entropy_cases import CASES, REFERENCED, SITUATIONS, case_image, case_offsets
from tests.resample_plan import Op
from tests.test_plan_host import run  # noqa: F401  (the fixture that builds and runs the plan driver)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP = Op(48, 64, True, "bilinear")  # the output the GPU test asks for (the plan's entropy half does not depend on it)
SMALL = {"alone": 1, "batch": 0}


def route_names(go) -> dict:
    """{value: name} of the unstuff and entropy routes (enum Route), as the driver's compiler sees them."""
    return {v: k for k, v in go.constants().items() if k.startswith("kRt")}


# -- the stage reference ---------------------------------------------------------------------------------------
def unstuff(jpg: bytes):
    """(segments, end): the unstuffed bytes of each restart segment of the first scan -- FF 00 gives FF, fill
    bytes and RSTn are dropped, RSTn begins a new segment -- and the code of the marker that ends the scan (None:
    the input ends first)."""
    scan = jpg[E.entropy_off(jpg):]
    segs, cur, pos, n = [], bytearray(), 0, len(scan)
    while True:
        i = scan.find(b"\xff", pos)
        if i < 0:
            cur += scan[pos:]
            end = None
            break
        cur += scan[pos:i]
        j = i + 1
        while j < n and scan[j] == 0xFF:
            j += 1
        if j >= n:
            end = None
            break
        m = scan[j]
        pos = j + 1
        if m == 0:
            cur.append(0xFF)
        elif 0xD0 <= m <= 0xD7:
            segs.append(bytes(cur))
            cur = bytearray()
        else:
            end = m
            break
    segs.append(bytes(cur))
    return segs, end


def reassemble(jpg: bytes) -> bytes:
    """A file with the same headers whose scan is written again from unstuff's segments."""
    segs, end = unstuff(jpg)
    assert end == 0xD9
    body = b"".join(s.replace(b"\xff", b"\xff\x00") + (bytes([0xFF, 0xD0 + k % 8]) if k + 1 < len(segs) else b"")
                    for k, s in enumerate(segs))
    return jpg[:E.entropy_off(jpg)] + body + b"\xff\xd9"


def pil_pixels(jpg: bytes) -> np.ndarray:
    from PIL import Image
    return np.array(Image.open(io.BytesIO(jpg)).convert("RGB"))


def total_blocks(jpg: bytes) -> int:
    """Blocks of the scan, from SOF0's sampling factors."""
    i = jpg.index(b"\xff\xc0")
    h, w, nc = int.from_bytes(jpg[i + 5:i + 7], "big"), int.from_bytes(jpg[i + 7:i + 9], "big"), jpg[i + 9]
    hv = [(jpg[i + 11 + 3 * c] >> 4, jpg[i + 11 + 3 * c] & 15) for c in range(nc)]
    if nc == 1:
        return -(-w // 8) * -(-h // 8)
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    return -(-w // (8 * hmax)) * -(-h // (8 * vmax)) * sum(a * b for a, b in hv)


def layout(segs, sub_bits: int, nsub_cap: int):
    """(nsub, first_at) of the subsequence layout (entspec_image): a segment of b bits takes max(1, ceil(b /
    sub_bits)) subsequences, nsub_cap at the most in all."""
    first_at, n = set(), 0
    for s in segs:
        first_at.add(n)
        n += max(1, -(-len(s) * 8 // sub_bits))
    return min(n, nsub_cap), first_at


def props_of(jpg: bytes, row, routes: dict) -> dict:
    """The fields the situations' conditions read: the driver's row and what follows from the unstuffed segments."""
    assert row.status == 0
    p = dict(row.ent)
    p["us"], p["ent"] = routes[row.routes[0]], routes[row.routes[1]]
    segs, _ = unstuff(jpg)
    p["nsub"], p["first_at"] = layout(segs, p["sub_bits"], p["nsub_cap"])
    p["ulen"] = sum(map(len, segs))
    p["useg"] = len(segs)
    p["bits_over_sub"] = -(-p["ulen"] * 8 // p["sub_bits"])
    p["blocks_per_sub"] = total_blocks(jpg) / p["nsub"]
    p["entropy_off_mod16"] = E.entropy_off(jpg) % 16
    return p


_PLANS: dict = {}


def plan_table(go) -> dict:
    """{(case name, mode): props}: every case planned with small = 0 (batch) and 1 (alone), once per process.
    go: test_plan_host.build_driver's -- the sanitized one here, a plain build for the GPU test."""
    if not _PLANS:
        keys = [(c, m) for c in CASES for m in ("alone", "batch")]
        rows = go([H.record(OP, SMALL[m], H.JPEG, case_image(c)) for c, m in keys])
        routes = route_names(go)
        for (c, m), row in zip(keys, rows):
            _PLANS[c.name, m] = props_of(case_image(c), row, routes)
    return _PLANS


@pytest.fixture(scope="module")
def plans(run):  # noqa: F811
    return plan_table(run)


# -- what this table and tests/gpu_debug.py read from the sources, against the compiler -------------------------
def test_constants_read_by_name_equal_the_compilers(run):  # noqa: F811
    """entropy_cases.const reads the headers as text; the driver prints the same names as compiled."""
    import ctypes

    from tests.gpu_debug import SubStateC
    k = run.constants()
    names = [n for n in k if n.startswith("k") and not n.startswith("kRt")]
    assert len(names) >= 14
    for n in names:
        assert E.const(n) == k[n], n
    assert E.const("SDSJ_REC_STORE", "sdsj_entropy.hip") <= k["kRec"]  # (sdsj_entropy.hip's own static_assert)
    assert ctypes.sizeof(SubStateC) == k["sizeof(SubState)"]
    for f in ("start_bit", "end_bit", "first", "seg"):
        assert getattr(SubStateC, f).offset == k[f"offsetof(SubState, {f})"], f


# -- the table's contract --------------------------------------------------------------------------------------
def test_case_names_are_unique():
    names = [c.name for c in CASES]
    assert len(names) == len(set(names))
    assert all(s in SITUATIONS for c in CASES for s in c.pins) and all(c.pins for c in CASES)


def test_table_holds_every_situation():
    pinned = {s for c in CASES for s in c.pins}
    assert pinned == set(SITUATIONS), set(SITUATIONS) - pinned
    # the group-count situations: 1 | 2, a count that does not divide, the cap -- in both plans, with restart
    # intervals and without; and every other edge by name, so that removing one from SITUATIONS fails too
    for tag in ("thr", "lat"):
        for what in ("g1", "g2", "gmid", "cap"):
            for r in ("rst", "norst"):
                assert f"{tag}_{what}_{r}" in pinned
    for s in ("empty_share_batch", "sync_pressure", "sync_control_batch", "seg_first_63", "seg_first_64", "seg_first_65",
              "nseg_over_256", "rec_many", "rec_few", "ent10_multi_group", "ent10_restart", "mh_on", "mh_off_restart",
              "straddle_serial", "straddle_serial_size_tile_parallel", "straddle_tile_parallel", "tiles_64", "tiles_65"):
        assert s in pinned, s
    assert sum(s.startswith("entropy_off_mod16_") for s in pinned) == 16


def test_the_truncated_set():
    """The cases the GPU test also runs cut at 2/3: a multi-group one, the empty-share one, the sync-pressure one."""
    cut = [c for c in CASES if c.truncate]
    assert {"empty_share_420", "sync_pressure_444"} < {c.name for c in cut} and len(cut) == 3
    (multi,) = [c for c in cut if c.name.startswith("noise_")]
    assert any(s.startswith("thr_g2") for s in multi.pins)


def test_referenced_situations_are_asserted_where_the_table_says():
    for name, (path, test, text) in REFERENCED.items():
        src = open(os.path.join(REPO, path)).read()
        body = src[src.index(f"def {test}("):]
        assert text in body, (name, path)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_has_its_plan(plans, case):
    for mode in ("alone", "batch"):
        p = plans[case.name, mode]
        assert p["lat"] == SMALL[mode]
        assert p["warm_small"] == p["warm_bits"] if p["lat"] else p["warm_small"] >= p["warm_bits"]
        for s in case.pins:
            if SITUATIONS[s][0] == mode:
                E.check(p, SITUATIONS[s][1], runtime=False, what=f"{case.name} [{mode}] {s}")
    if not case.big:
        i = case_image(case).index(b"\xff\xc0")
        h, w = (int.from_bytes(case_image(case)[i + k:i + k + 2], "big") for k in (5, 7))
        assert w * h <= 1 << 20, "only the cap cases may exceed 1 MP"


# -- byte-level properties -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c.group == "straddle"], ids=lambda c: c.name)
def test_straddled_pairs_sit_on_the_boundaries(case):
    jpg, found = case_image(case), case_offsets(case)
    scan = jpg[E.entropy_off(jpg):]
    assert [(k, m) for k, m, _ in found] == list(E.STRADDLES)
    assert E.const("kUsTileBytes") == 8192
    for kind, mod, x in found:
        assert x % mod == 0 and (mod == 8192 or x % 8192 != 0), (kind, mod, x)
        assert scan[x - 1] == 0xFF
        if kind == "ff00":
            assert scan[x] == 0 and scan[x - 2] != 0xFF
        elif kind == "rst":
            assert 0xD0 <= scan[x] <= 0xD7 and scan[x - 2] != 0xFF
        else:
            assert 0xD0 <= scan[x] <= 0xD7 and scan[x - 2] == 0xFF and scan[x - 3] != 0xFF
    assert pil_pixels(jpg).shape[2] == 3


def test_fill_padding():
    (case,) = [c for c in CASES if c.group == "padded"]
    jpg, twin = case_image(case), case.twin()
    assert len(jpg) - len(twin) == 3 * 350000
    assert jpg.replace(b"\xff" * 350000, b"") == twin
    for pos in E.rst_positions(jpg):
        assert jpg[pos - 350000:pos] == b"\xff" * 350000
    assert unstuff(jpg) == unstuff(twin)
    np.testing.assert_array_equal(pil_pixels(jpg), pil_pixels(twin))


def test_scan_start_residues():
    cs = [c for c in CASES if c.group == "residue"]
    assert sorted(E.entropy_off(case_image(c)) % 16 for c in cs) == list(range(16))
    ref = pil_pixels(case_image(cs[0]))
    scans = {case_image(c)[E.entropy_off(case_image(c)):] for c in cs}
    assert len(scans) == 1  # one small image, emitted 16 times
    for c in cs:
        np.testing.assert_array_equal(pil_pixels(case_image(c)), ref)


@pytest.mark.parametrize("case", [c for c in CASES if c.group == "same_coef"], ids=lambda c: c.name)
def test_restart_twin_has_the_same_coefficients(case):
    np.testing.assert_array_equal(pil_pixels(case_image(case)), pil_pixels(case.twin()))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_restated_unstuffing_against_pil(case):
    """PIL decodes the file written again from the restatement's segments to the pixels of the original.  (The
    cap cases, PIL noise files without fill bytes, must come back byte for byte; they are not decoded.)"""
    jpg = case_image(case)
    again = reassemble(jpg)
    if case.big:
        assert again == jpg and len(unstuff(jpg)[0]) == plan_nseg(jpg)
        return
    if case.group in ("padded", "straddle") or "tiles_6" in case.name:
        assert len(again) < len(jpg)  # (the fill bytes are gone)
    else:
        assert again == jpg
    np.testing.assert_array_equal(pil_pixels(again), pil_pixels(jpg))
    assert len(unstuff(jpg)[0]) == plan_nseg(jpg)


def plan_nseg(jpg: bytes) -> int:
    """Restart intervals of the scan: ceil(MCUs / DRI's interval), 1 without DRI."""
    i = jpg.find(b"\xff\xdd\x00\x04")
    if i < 0 or i > E.entropy_off(jpg):
        return 1
    ri = int.from_bytes(jpg[i + 4:i + 6], "big")
    s = jpg.index(b"\xff\xc0")
    h, w, nc = int.from_bytes(jpg[s + 5:s + 7], "big"), int.from_bytes(jpg[s + 7:s + 9], "big"), jpg[s + 9]
    hmax = max(jpg[s + 11 + 3 * c] >> 4 for c in range(nc)) if nc > 1 else 1
    vmax = max(jpg[s + 11 + 3 * c] & 15 for c in range(nc)) if nc > 1 else 1
    return -(-(-(-w // (8 * hmax)) * -(-h // (8 * vmax))) // ri)
