"""CPU restatement of the resample plan (test infrastructure: a checker, never imported by sds_amd).

Restates, in Python doubles with the C code's operation order, what decides the resample kernel an image
gets: ``setup_geometry``'s component sizes, ``crop_box``, ``resample_ksize`` and ``filter_support``
(sds_amd/csrc/sdsj_common.h), the tile-halving loop and the ``rs_*`` limits of ``plan_image`` and
``image_routes`` (sds_amd/csrc/sdsj_plan.h), the lane split of ``run_chunk``
(sds_amd/csrc/sdsj_engine.hip) and the strip height of ``launch_resample`` (sds_amd/csrc/sdsj_resample.hip).
tests/test_plan_host.py compares it with the C++ planner on the CPU, tests/test_gpu_resample_routes.py with
the device's descriptors.

    p = plan(600, 450, S422, Op(400, 300))
    p.route_name          # 'kRtF_422_5'  (kRtF + lay * 5 + (kt - 3) / 2: k_rs420<5, 4:2:2>)
    p.tiles               # 2
    strip_h(600, lanes=1) # 64
"""
from __future__ import annotations

from dataclasses import dataclass

# sdsj_common.h
K_MAX_SPAN = 960
K_RING_DW = 3072
K_RING_MAX_ROWS = 16
K_VTAPS_F = 16
K_MAX_STRIP = 64          # sdsj_pixel.h
K_LANE_MIN, K_MAX_LANES = 128, 4  # sdsj_engine.hip
GEO_RESIZE, GEO_IDENTITY, GEO_ZEROS = 0, 1, 2
LAY_420, LAY_422, LAY_444, LAY_GRAY = 0, 1, 2, 3
LAY_NAMES = ("420", "422", "444", "gray")
SPEC_TAPS = (3, 5, 7, 9, 11)

# enum Route, the resample part: kRtUnfused, kRtGen0, kRtGen1, kRtGen3 .. kRtGen11, then kRtF + 0 .. 19
RT_UNFUSED, RT_GEN0, RT_GEN1, RT_GEN3 = 0, 1, 2, 3
RT_F = 8
ROUTE_NAMES = ["kRtUnfused", "kRtGen0", "kRtGen1", "kRtGen3", "kRtGen5", "kRtGen7", "kRtGen9", "kRtGen11"] + \
              [f"kRtF_{lay}_{kt}" for lay in LAY_NAMES for kt in SPEC_TAPS]
assert len(ROUTE_NAMES) == 28

FILTER_SUPPORT = {"box": 0.5, "bilinear": 1.0, "hamming": 1.0, "bicubic": 2.0, "lanczos": 3.0}

# per-component (h, v) sampling factors
S420 = ((2, 2), (1, 1), (1, 1))
S422 = ((2, 1), (1, 1), (1, 1))
S444 = ((1, 1), (1, 1), (1, 1))
S440 = ((1, 2), (1, 1), (1, 1))
GRAY = ((1, 1),)


@dataclass(frozen=True)
class Op:
    out_h: int
    out_w: int
    crop: bool = True
    filter: str = "bilinear"


@dataclass(frozen=True)
class Plan:
    geo: int
    cx0: int
    cy0: int
    cw: int
    ch: int
    need_h: int
    need_v: int
    ksh: int
    ksv: int
    ring_rows: int
    fused: int
    tile_w: int
    rs_fast: int
    rs_lay: int
    route: int       # -1: an empty crop (zeros, no resample kernel)
    tiles: int       # column tiles of a fused route (out_w > tile_w <=> tiles > 1)
    span: float      # plan_image's source-column bound of one tile (0 when not fused)
    max_hc: int      # widest horizontal / vertical window over the output's columns / rows (0: no pass)
    max_vc: int

    @property
    def route_name(self) -> str:
        return ROUTE_NAMES[self.route] if self.route >= 0 else "none"

    @property
    def multi_tile(self) -> bool:
        return self.tiles > 1


def rs_ring_rows(kt): return 8 if kt <= 7 else K_RING_MAX_ROWS
def rs_vtaps(kt): return 8 if kt <= 7 else K_VTAPS_F
def rs_ring_dw(kt): return 8 * 256 if kt <= 7 else K_RING_DW
def rs_span(kt): return 768 if kt <= 7 else K_MAX_SPAN
def rs_route(lay, kt): return RT_F + lay * 5 + (kt - 3) // 2


def gen_route(kt):
    if kt == 1:
        return RT_GEN1
    return RT_GEN3 + (kt - 3) // 2 if 3 <= kt <= 11 and kt & 1 else RT_GEN0


def _tdiv(a: int, b: int) -> int:
    """C integer division (truncates towards zero)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def ceil_div(a, b): return (a + b - 1) // b


def crop_box(w, h, out_h, out_w):
    cur = float(w) / float(h)
    tgt = float(out_w) / float(out_h)
    if cur > tgt:
        nw = int(float(h) * tgt)
        return _tdiv(w - nw, 2), 0, nw, h
    nh = int(float(w) / tgt)
    return 0, _tdiv(h - nh, 2), w, nh


def resample_ksize(in_size, out_size, support):
    scale = float(in_size) / out_size
    fs = 1.0 if scale < 1.0 else scale
    s = support * fs
    c = int(s)
    if float(c) < s:
        c += 1
    return c * 2 + 1


def window_counts(in_size, out_size, support) -> list[int]:
    """Taps Pillow's precompute_coeffs gives each output index (resample_bounds): at most
    ceil(2 x support x max(scale, 1)), one fewer than resample_ksize -- the last tap of a KT-tap kernel
    never carries a weight, the one before it only for the widest windows."""
    scale = float(in_size) / out_size
    s = support * (1.0 if scale < 1.0 else scale)
    out = []
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - s + 0.5), 0)
        xmax = min(int(center + s + 0.5), in_size)
        out.append(xmax - xmin)
    return out


def components(width, height, sampling):
    """Per component (rh, rv, dw, dh) as setup_geometry derives them."""
    hmax = max(h for h, _ in sampling)
    vmax = max(v for _, v in sampling)
    out = []
    for h, v in sampling:
        assert hmax % h == 0 and vmax % v == 0 and hmax // h <= 2 and vmax // v <= 2, "unsupported sampling"
        out.append((hmax // h, vmax // v, ceil_div(width * h, hmax), ceil_div(height * v, vmax)))
    return out


def resample_route(geo, fused, rs_fast, rs_lay, need_h, ksh) -> int:
    """image_routes' resample route of a planned JPEG (-1: an empty crop), from the descriptor's fields."""
    if geo == GEO_ZEROS:
        return -1
    if not fused:
        return RT_UNFUSED
    return rs_route(rs_lay, rs_fast) if rs_fast else gen_route(ksh if need_h else 1)


def plan(width: int, height: int, sampling, op: Op) -> Plan:
    """plan_image + image_routes for a baseline JPEG (no frames, PNG or NEAREST: those take the unfused
    passes under their own tests)."""
    assert len(sampling) in (1, 3) and op.filter in FILTER_SUPPORT
    comp = components(width, height, sampling)
    W, H = width, height
    if W == op.out_w and H == op.out_h:
        geo, (cx0, cy0, cw, ch) = GEO_IDENTITY, (0, 0, W, H)
    else:
        geo = GEO_RESIZE
        cx0, cy0, cw, ch = crop_box(W, H, op.out_h, op.out_w) if op.crop else (0, 0, W, H)
        if cw <= 0 or ch <= 0:
            geo = GEO_ZEROS
    need_h = int(geo == GEO_RESIZE and cw != op.out_w)
    need_v = int(geo == GEO_RESIZE and ch != op.out_h)
    sup = FILTER_SUPPORT[op.filter]
    ksh = resample_ksize(cw, op.out_w, sup) if need_h else 0
    ksv = resample_ksize(ch, op.out_h, sup) if need_v else 0
    fused, tile_w, span = 0, 0, 0.0
    ring_rows = 1
    while ring_rows < ksv:
        ring_rows *= 2
    if geo != GEO_ZEROS and ring_rows <= K_RING_MAX_ROWS:
        scale = float(cw) / op.out_w if need_h else 1.0
        supp = sup * (1.0 if scale < 1.0 else scale) if need_h else 0.0
        tw = op.out_w if op.out_w < 256 else 256
        if tw > K_RING_DW // ring_rows:
            tw = K_RING_DW // ring_rows
        lim = rs_span(ksh) if ksh <= 7 else K_MAX_SPAN
        while True:
            span = float(tw) * scale + 2.0 * supp + 4.0
            if span <= float(lim):
                fused, tile_w = 1, tw
                break
            if tw == 1:
                break
            tw = (tw + 1) // 2
    rs_fast, rs_lay = 0, LAY_420
    if fused and need_h and need_v and 3 <= ksh <= 11 and ksh & 1 and ring_rows <= rs_ring_rows(ksh) and \
            ksv <= rs_vtaps(ksh) and tile_w * ring_rows <= rs_ring_dw(ksh) and span <= float(rs_span(ksh)) and \
            comp[0][0] == 1 and comp[0][1] == 1:
        lay = -1
        if len(comp) == 1:
            lay = LAY_GRAY
        else:
            c1, c2 = comp[1], comp[2]
            same = c1 == c2
            if same and c1[0] == 1 and c1[1] == 1:
                lay = LAY_444
            elif same and c1[0] == 2 and c1[1] == 1 and c1[2] > 2:
                lay = LAY_422
            elif same and c1[0] == 2 and c1[1] == 2 and c1[2] > 2:
                lay = LAY_420
        if lay >= 0:
            rs_fast, rs_lay = ksh, lay
    route = resample_route(geo, fused, rs_fast, rs_lay, need_h, ksh)
    tiles = ceil_div(op.out_w, tile_w) if fused else 0
    return Plan(geo, cx0, cy0, cw, ch, need_h, need_v, ksh, ksv, ring_rows, fused, tile_w, rs_fast, rs_lay, route, tiles,
                span if fused else 0.0,
                max(window_counts(cw, op.out_w, sup)) if need_h else 0,
                max(window_counts(ch, op.out_h, sup)) if need_v else 0)


def lane_sizes(batch: int, lanes: int = 4) -> list[int]:
    """Images per lane of one chunk of `batch` images (run_chunk)."""
    nl = min(max(lanes, 1), K_MAX_LANES)
    while nl > 1 and batch < nl * K_LANE_MIN:
        nl -= 1
    return [batch * (k + 1) // nl - batch * k // nl for k in range(nl)]


def strip_h(batch: int, lanes: int = 4) -> list[int]:
    """Output rows per fused-resample strip, per lane: launch_resample's n is the lane's image count."""
    return [K_MAX_STRIP if n >= 512 else 16 for n in lane_sizes(batch, lanes)]


def generic_step_rows(width: int, height: int, sampling, ax0: int, ax1: int) -> int:
    """Rows per step of k_resample's tile over image columns [ax0, ax1) (resample_tile's rs loop): the
    staging pool of kStageDW = 2944 dwords holds, per component, rs rows (rs / 2 + 2 when it is
    v-subsampled) of nd dwords."""
    comp = components(width, height, sampling)
    nds = []
    for rh, _, dw, _ in comp:
        lo, hi = ax0, ax1 - 1
        if rh == 2:
            lo, hi = max((ax0 >> 1) - 1, 0), min(((ax1 - 1) >> 1) + 1, dw - 1)
        jal = lo & ~3
        nds.append((hi + 1 - jal + 3) >> 2)
    rs = 4
    while True:
        need = sum((rs // 2 + 2 if c[1] == 2 else rs) * nd for c, nd in zip(comp, nds))
        if need <= 2944 or rs == 1:
            return rs
        rs -= 1
