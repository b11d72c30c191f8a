"""Host AddressSanitizer + UBSan run of the planner (sds_amd/csrc/sdsj_plan.h): plan_sample -- the format
dispatch, header parse, geometry and plan_image that k_parse lane 0 and host planning run -- and
image_routes, in a stand-alone program (tests/asan/plan_driver.cpp, its own main).  plan_image decides
every scratch offset the later kernels trust, image_routes the kernel an image gets.

1. The restatement (tests/resample_plan.py) is pinned to the C++ on the CPU: for every case of the route
   table the comparisons tests/test_gpu_resample_routes.py check_plan makes on the device's descriptors.
2. The scratch layout of every planned sample: 256-byte aligned offsets in plan_image's order, inside need.
3. The damaged inputs of tests/test_asan_parser.py go through plan_sample without a sanitizer report, and
   status and need equal the product library's sdsj_plan_need_formats where it is loadable."""
import ctypes
import os
import shutil
import struct
import subprocess
import tempfile

import pytest

from tests import goldens as G
from tests import png_synth as S
from tests import resample_plan as P
from tests.parser_inputs import inputs as damaged_inputs
from tests.resample_cases import CASES, case_image, strip_cases

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "asan", "plan_driver.cpp")

FILTERS = {"box": 0, "bilinear": 1, "hamming": 2, "bicubic": 3, "lanczos": 4, "nearest": 5}  # SDSJ_FILTER_*
JPEG, PNG = 1, 2  # SDSJ_FORMAT_*
RT_PNG = 35       # enum Route (sdsj_common.h); the driver prints the header's value
PLAN_FIELDS = ("geo", "cx0", "cy0", "cw", "ch", "need_h", "need_v", "ksh", "ksv", "ring_rows", "fused", "tile_w",
               "rs_fast", "rs_lay")  # as tests/test_gpu_resample_routes.py
OFFSETS = ("off_ustream", "off_seg", "off_tiles", "off_sub", "off_rec", "off_ptab", "off_coef", "off_planes", "off_rgb",
           "off_tmp", "off_kh", "off_kv", "off_png")  # plan_image's take order
LAYOUT_OPS = (P.Op(256, 256, True, "bilinear"), P.Op(512, 512, False, "bicubic"), P.Op(48, 64, True, "lanczos"),
              P.Op(100, 100, True, "nearest"))
# (warm_bits: plan_image's, for a lane of at least kWarmSmallLane images; warm_small: what k_parse gives below it)
ENT_FIELDS = ("entropy_len", "nseg", "ntiles", "sub_bits", "nsub_cap", "warm_bits", "ent_groups", "lat", "mh",
              "warm_small")  # the entropy / unstuff plan (tests/test_entropy_cases_table.py)
DAMAGE_OP = P.Op(256, 256, True, "bilinear")


class Row:
    def __init__(self, line: str):
        v = list(map(int, line.split()))
        assert len(v) == 1 + len(PLAN_FIELDS) + 3 + 1 + len(OFFSETS) + 3 + len(ENT_FIELDS), line
        self.status = v[0]
        self.plan = dict(zip(PLAN_FIELDS, v[1:15]))
        self.routes = tuple(v[15:18])  # unstuffing, entropy, resample
        self.need = v[18]
        self.offsets = v[19:32]
        self.size = tuple(v[32:35])    # width, height, ncomp
        self.ent = dict(zip(ENT_FIELDS, v[35:45]))


def record(op: P.Op, small: int, formats: int, data: bytes) -> bytes:
    return struct.pack("<6iI", op.out_h, op.out_w, int(op.crop), FILTERS[op.filter], small, formats, len(data)) + data


def build_driver(sanitize: bool = True):
    """Builds the driver; the returned run(records) plans them all in one process and returns their rows, and
    run.constants() returns what `plan_driver --constants` prints, {name: value}.  sanitize=False: the same
    program without the sanitizers, for callers that only need the rows (the GPU tests)."""
    d = tempfile.mkdtemp()
    exe = os.path.join(d, "plan_driver")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    r = subprocess.run(["g++", "-std=c++17", "-O1", *flags, "-I", os.path.join(HERE, "..", "include"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ)
    if sanitize:
        env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")

    def go(records):
        blob = os.path.join(d, "inputs.bin")
        with open(blob, "wb") as f:
            f.write(b"".join(records))
        r = subprocess.run([exe, blob], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        lines = r.stdout.splitlines()
        assert tuple(map(int, lines[0].split())) == (P.RT_UNFUSED, RT_PNG)
        assert len(lines) == 1 + len(records)
        return [Row(l) for l in lines[1:]]

    def constants():
        r = subprocess.run([exe, "--constants"], capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-4000:]
        return {k: int(v) for k, v in (l.rsplit(None, 1) for l in r.stdout.splitlines())}
    go.constants = constants
    return go


@pytest.fixture(scope="module")
def run():
    """Builds the sanitized driver once."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    return build_driver()


def test_restated_planner_equals_plan_image(run):
    cases = CASES + strip_cases()
    rows = run([record(c.op, 0, JPEG, case_image(c)) for c in cases])
    for c, row in zip(cases, rows):
        p = c.plan()
        assert row.status == 0, c.name
        assert row.size == (c.w, c.h, 1 if c.samp == "gray" else 3), c.name
        want = {f: getattr(p, f) for f in PLAN_FIELDS}
        assert row.plan == want, f"{c.name}: plan_image planned {row.plan}, the restatement {want}"
        d = row.plan
        route = P.resample_route(d["geo"], d["fused"], d["rs_fast"], d["rs_lay"], d["need_h"], d["ksh"])
        assert route == row.routes[2], c.name  # image_routes itself
        assert P.ROUTE_NAMES[route] == c.route, f"{c.name}: route {P.ROUTE_NAMES[route]}, intended {c.route}"
        assert bool(d["fused"] and -(-c.res[1] // d["tile_w"]) > 1) == c.multi, c.name


def _pngs():
    return [S.make(13, 7, 2, "mixP"), S.make(67, 5, 3, "mixA"), S.make(200, 129, 6, "mixU")]


def test_scratch_layout(run):
    # (data, formats, must plan: the case images and the PNGs do; a G1 golden may be one this path hands over)
    samples = [(x, JPEG, True) for x in dict.fromkeys(case_image(c) for c in CASES + strip_cases())]
    samples += [(jpg, JPEG, False) for _, jpg, _ in G.g1()]
    samples += [(x, JPEG | PNG, True) for x in _pngs()]
    keys = [(op, small, s) for op in LAYOUT_OPS for small in (0, 1) for s in samples]
    rows = run([record(op, small, fm, x) for op, small, (x, fm, _) in keys])
    n_ok = 0
    for (op, small, (x, fm, must)), row in zip(keys, rows):
        what = (op, small, fm, len(x), row.size)
        assert row.status == 0 or not must, what
        if row.status != 0:
            assert row.need == 0, what
            continue
        n_ok += 1
        assert all(o % 256 == 0 and o >= 0 for o in row.offsets), (what, row.offsets)
        assert all(a <= b for a, b in zip(row.offsets, row.offsets[1:])), (what, row.offsets)
        assert row.need % 256 == 0 and row.need >= row.offsets[-1] and row.need > 0, (what, row.need, row.offsets)
        if fm & PNG:
            assert row.routes == (-1, RT_PNG, P.RT_UNFUSED), (what, row.routes)
    assert n_ok >= sum(must for _, _, must in samples) * len(LAYOUT_OPS) * 2


def test_damaged_inputs(run):
    inputs = damaged_inputs()
    keys = [(fm, x) for fm in (JPEG, JPEG | PNG) for x in inputs]
    rows = run([record(DAMAGE_OP, 0, fm, x) for fm, x in keys])
    assert all((r.status == 0) == (r.need > 0) for r in rows)
    assert any(r.status == 0 for r in rows) and any(r.status != 0 for r in rows)
    try:
        from sds_amd import _lib
        lib = _lib.load()
    except Exception:  # noqa: BLE001  (the product library is not built: the sanitizers' verdict only)
        return
    op = _lib.SdsjOp(DAMAGE_OP.out_h, DAMAGE_OP.out_w, 1, FILTERS[DAMAGE_OP.filter], 0, 0)
    for (fm, x), row in zip(keys, rows):
        need = ctypes.c_int64(-1)
        st = lib.sdsj_plan_need_formats(x, len(x), ctypes.byref(op), fm, ctypes.byref(need))
        assert (st, need.value) == (row.status, row.need), (fm, len(x), st, need.value, row.status, row.need)
