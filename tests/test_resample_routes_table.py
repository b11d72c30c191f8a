"""The resample route case table (tests/resample_cases.py), proved on the CPU with the restated planner
(tests/resample_plan.py): every case lands on its intended route, and the table holds every route and
every group the GPU run (tests/test_gpu_resample_routes.py) relies on.  The conditions below are the
table's contract: an entry that stops satisfying one fails here, without a GPU."""
import os

import pytest

from tests import resample_plan as P
from tests.resample_cases import CASES, STRIP_BATCH, STRIP_IMAGES, STRIP_OPS, strip_cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN_K = ["kRtGen3", "kRtGen5", "kRtGen7", "kRtGen9", "kRtGen11"]


def test_restated_planner_on_known_plans():
    """The restatement on plans the kernel sources state themselves."""
    # sdsj_common.h rs_span: bilinear scales in (2.97, 3] halve the 256-column tile of the 7-tap kernels
    assert P.plan(755, 755, P.S420, P.Op(256, 256)).tile_w == 256
    assert P.plan(768, 768, P.S420, P.Op(256, 256)).tile_w == 128
    p = P.plan(771, 771, P.S420, P.Op(256, 256))  # the 9-tap neighbour just past scale 3: 960-column rows
    assert (p.ksh, p.tile_w, p.route_name) == (9, 192, "kRtF_420_9")
    # the flagship: VGA 4:2:0 to 256 x 256 is k_rs420<5, 4:2:0>, one tile
    p = P.plan(640, 480, P.S420, P.Op(256, 256))
    assert (p.cx0, p.cy0, p.cw, p.ch, p.ksh, p.ksv, p.route_name, p.tiles) == (80, 0, 480, 480, 5, 5, "kRtF_420_5", 1)
    assert P.crop_box(128, 96, 48, 48) == (16, 0, 96, 96)
    assert P.strip_h(512, lanes=4) == [16] * 4 and P.strip_h(512, lanes=1) == [64] and P.strip_h(511, lanes=1) == [16]
    assert P.lane_sizes(640) == [160] * 4 and P.lane_sizes(300) == [150, 150] and P.lane_sizes(40) == [40]


@pytest.mark.parametrize("case", CASES + strip_cases(), ids=lambda c: c.name)
def test_case_lands_on_its_route(case):
    p = case.plan()
    assert p.route_name == case.route, (case.name, p)
    assert p.multi_tile == case.multi, (case.name, p.tile_w, p.tiles)
    assert p.geo != P.GEO_ZEROS


def test_case_names_are_unique():
    names = [c.name for c in CASES + strip_cases()]
    assert len(names) == len(set(names))


def test_table_holds_all_28_routes():
    assert {c.route for c in CASES} == set(P.ROUTE_NAMES)
    assert len(P.ROUTE_NAMES) == 28


def test_every_specialised_route_single_and_multi_tile():
    for lay in P.LAY_NAMES:
        for kt in P.SPEC_TAPS:
            hits = [c for c in CASES if c.route == f"kRtF_{lay}_{kt}"]
            assert any(not c.plan().multi_tile for c in hits), (lay, kt, "single-tile")
            multi = [c for c in hits if c.plan().multi_tile]
            assert multi, (lay, kt, "multi-tile")
            for c in multi:
                p = c.plan()
                assert c.res[1] > p.tile_w and (kt > 5 or c.res[1] > 256)
    # every specialised kernel once with the widest windows Pillow builds for its tap count, KT - 1 taps,
    # in both passes (the KT-th tap never carries a weight: resample_plan.window_counts), single- and multi-tile
    for lay in P.LAY_NAMES:
        for kt in P.SPEC_TAPS:
            for multi in (False, True):
                assert any(c.plan().max_hc == kt - 1 and c.plan().max_vc == c.plan().ksv - 1
                           for c in CASES if c.route == f"kRtF_{lay}_{kt}" and c.multi == multi), (lay, kt, multi)
    for c in CASES:
        assert c.plan().max_hc <= max(c.plan().ksh - 1, 0) and c.plan().max_vc <= max(c.plan().ksv - 1, 0)
    for kt in P.SPEC_TAPS:  # every tap count also through a filter other than bilinear
        assert any(c.filter != "bilinear" and c.plan().rs_fast == kt for c in CASES), kt
    # KT = 11 through bilinear, as 288 x 216 -> (48, 64)
    assert any(c.filter == "bilinear" and c.plan().rs_fast == 11 and (c.w, c.h, c.res) == (288, 216, (48, 64)) for c in CASES)


def test_generic_routes():
    by = {r: [c for c in CASES if c.route == r] for r in ["kRtGen0", "kRtGen1", "kRtUnfused"] + GEN_K}
    # kRtGen1: vertical-only (the crop keeps the width), and the same-size shortcut
    plans = [c.plan() for c in by["kRtGen1"]]
    assert any(p.geo == P.GEO_RESIZE and not p.need_h and p.need_v and p.cw == c.res[1]
               for p, c in zip(plans, by["kRtGen1"]))
    assert any(p.geo == P.GEO_IDENTITY for p in plans)
    for r in GEN_K + ["kRtGen0"]:
        assert any(not c.plan().multi_tile for c in by[r]), (r, "single-tile")
    assert any(c.plan().multi_tile for c in by["kRtGen0"])
    assert any(c.plan().multi_tile for r in GEN_K for c in by[r])
    assert all(c.plan().ksh >= 13 for c in by["kRtGen0"])
    for r in GEN_K:  # ... and with the widest window of its tap count (KT - 1 taps carry a weight)
        assert any(c.plan().max_hc == c.plan().ksh - 1 for c in by[r]), (r, "widest window")
    # the ways in: 4:4:0, horizontal-only, a vertical window past the specialised kernels', chroma dw <= 2
    gen = [c for r in GEN_K + ["kRtGen0"] for c in by[r]]
    assert any(c.samp == "440" for c in gen)
    assert any(c.plan().need_h and not c.plan().need_v for c in gen)
    assert any(c.samp != "440" and c.plan().need_v and c.plan().ksv > P.rs_vtaps(c.plan().ksh) for c in gen)
    assert any(c.samp in ("420", "422") and P.components(c.w, c.h, P.S420)[1][2] <= 2 for c in gen)
    assert (200, 400, (100, 100), False) in [(c.w, c.h, c.res, c.crop) for c in by["kRtGen5"]]
    assert (700, 200, (100, 100), False) in [(c.w, c.h, c.res, c.crop) for c in by["kRtGen0"]]
    # unfused: a JPEG whose vertical window is longer than the ring
    assert any(c.plan().ksv > P.K_RING_MAX_ROWS and not c.plan().fused for c in by["kRtUnfused"])
    assert (300, 900, (100, 100), False) in [(c.w, c.h, c.res, c.crop) for c in by["kRtUnfused"]]


def test_generic_tile_at_the_960_column_bound():
    """4:4:4 and 4:4:0 generic tiles whose source-column bound sits within 4 columns of kMaxSpan.  There
    the staging pool decides the rows per step (resample_tile's rs loop) -- and never shortens it: a tile
    of at most 960 columns stages at most (960 + 3 + 3) / 4 = 241 dwords per row (the first column
    rounded down and the last up to a dword), and 3 components x 4 rows (a v-subsampled component's
    rs / 2 + 2 rows are 4 as well) x 241 = 2892 <= kStageDW = 2944.  So no case takes the shorter step."""
    cs = [c for c in CASES if c.group == "span960"]
    assert {c.samp for c in cs} == {"444", "440"}
    for c in cs:
        p = c.plan()
        assert p.fused and not p.rs_fast and P.K_MAX_SPAN - 4 < p.span <= P.K_MAX_SPAN, (c.name, p.span)
        scale = p.cw / c.res[1]
        for tile in range(p.tiles):  # the tile's image columns, bounded by the image
            ax0 = max(int(tile * p.tile_w * scale) - 8, 0)
            ax1 = min(ax0 + P.K_MAX_SPAN, c.w)
            assert P.generic_step_rows(c.w, c.h, P.S444 if c.samp == "444" else P.S440, ax0, ax1) == 4
    assert 3 * 4 * ((P.K_MAX_SPAN + 3 + 3) // 4) <= 2944
    for samp in (P.S444, P.S440, P.S420, P.S422):
        for ax0 in range(0, 8):
            assert P.generic_step_rows(4000, 64, samp, ax0, ax0 + P.K_MAX_SPAN) == 4


def test_crop_boxes_around_chroma_block_boundaries():
    for lay in ("420", "422", "440"):
        cs = [c for c in CASES if c.group == "edge" and c.samp == lay]
        boxes = [(c.plan().cx0, c.plan().cy0, c.plan().cw, c.plan().ch) for c in cs]
        for e in (15, 16, 17):  # one before, on and one after the boundary at 16; the far edge 96 on
            assert (e, 0, 96, 96) in boxes, (lay, "left edge", e)
            assert (0, e, 96, 96) in boxes, (lay, "top edge", e)
        assert all(c.crop and c.res[0] == c.res[1] for c in cs)


def test_64_row_strip_group():
    cs = strip_cases()
    assert {c.res[0] for c in cs} == {65, 130}  # two strips with a 1-row tail; three with a 2-row tail
    assert P.strip_h(STRIP_BATCH, lanes=1) == [P.K_MAX_STRIP]
    assert all(-(-c.res[0] // P.K_MAX_STRIP) >= 2 and c.res[0] % P.K_MAX_STRIP for c in cs)
    assert 8 <= len(set(STRIP_IMAGES)) <= 16 and len(set(STRIP_IMAGES)) == len(STRIP_IMAGES)
    assert all(w <= 100 and h <= 100 for _, w, h in STRIP_IMAGES)
    for res, filt in STRIP_OPS:
        assert {c.samp for c in cs if c.res == res and c.filter == filt} == {"420", "422", "444", "gray", "440"}
    routes = {c.route for c in cs}
    assert all(c.plan().fused for c in cs)
    # kernels that run 64-row strips here: specialised ones of every layout, and the generic one
    assert {r.split("_")[1] for r in routes if r.startswith("kRtF_")} == set(P.LAY_NAMES)
    assert any(r.startswith("kRtGen") for r in routes)


def test_the_product_does_not_import_the_restatement():
    for root, _, files in os.walk(os.path.join(REPO, "sds_amd")):
        for f in files:
            if f.endswith(".py"):
                with open(os.path.join(root, f)) as fh:
                    src = fh.read()
                assert "resample_plan" not in src and "resample_cases" not in src, f
