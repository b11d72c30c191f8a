"""Every resample kernel route on the GPU: the device's plan against the restated planner, the pixels
against the oracle.

The cases come from tests/resample_cases.py (tests/test_resample_routes_table.py proves on the CPU that they
cover all 28 routes, single- and multi-tile, the chroma-block-boundary crops and the 64-row strips).  For
every case the chunk's descriptors are read back (tests/gpu_debug.py snapshot) and geo, crop box, ksh, ksv,
fused, tile_w, ring_rows, rs_fast and rs_lay must equal the restatement's -- so the route is the intended
one: a case that slides to another kernel fails here.  Outputs equal ``O.pipeline`` bit for bit (tolerance
0), in two output forms (uint8 / CHW / unflipped and float32-normalised / HWC / flipped: each kernel has its
own OutMap write path), every case alone (a latency-mode chunk) and inside a batch of more than 32 mixed
images (the throughput plan).

Dirtied scratch: before every decode the same engine decodes a batch of noise JPEGs whose total scratch
need is larger (asserted), so the planes, tables and rows the case then uses hold unrelated non-zero bytes,
and a case's own image is never decoded at another geometry first.  k_entwrite / k_idct produce only the
blocks the crop needs; whatever the fused kernels stage beyond them must feed no pixel of the tile."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)
from tests import gpu_debug  # noqa: E402
from tests import resample_plan as P  # noqa: E402
from tests.resample_cases import (CASES, STRIP_BATCH, STRIP_IMAGES, STRIP_OPS, Case, case_image,  # noqa: E402
                                  strip_cases)

# (normalize, layout, flip)
FORMS = ((False, "chw", False), (True, "hwc", True))
PLAN_FIELDS = ("geo", "cx0", "cy0", "cw", "ch", "need_h", "need_v", "ksh", "ksv", "ring_rows", "fused", "tile_w",
               "rs_fast", "rs_lay")
OK_COUNTERS = ("unsupported", "corrupt", "capacity", "other")


class Rig:
    def __init__(self):
        from sds_amd.engine import JpegEngine
        from tests.golden.synth import encode_jpeg
        self.engine = JpegEngine(max_batch=STRIP_BATCH)
        rng = np.random.default_rng(2024)
        noise = [encode_jpeg(rng.integers(0, 256, (480, 640, 3), dtype=np.uint8), 95) for _ in range(4)]
        self.noise = [noise[k % 4] for k in range(24)]
        self.refs = {}

    def dirty(self) -> int:
        """Decodes the noise batch; returns the scratch bytes it took (the next decode must take fewer)."""
        _, st = self.engine.decode_resize(self.noise, (32, 32))
        assert (st == 0).all()
        descs, _ = gpu_debug.snapshot(self.engine, len(self.noise))
        return sum(d.need for d in descs)

    def ref(self, case: Case, form) -> np.ndarray:
        """The oracle's output of a case, computed once per (image, op) and shared read-only."""
        key = (case.samp, case.w, case.h, case.content, case.op)
        if key not in self.refs:
            r = O.pipeline(case_image(case), case.res, crop_before_resize=case.crop, filter=case.filter)
            r.setflags(write=False)
            self.refs[key] = r
        chw = self.refs[key]
        normalize, layout, flip = form
        if flip:
            chw = chw[:, :, ::-1]
        if normalize:
            chw = O.normalize_lut()[chw]
        return np.ascontiguousarray(chw.transpose(1, 2, 0) if layout == "hwc" else chw)

    def run(self, cases, form):
        """Dirties the scratch, decodes the cases as one chunk in the given output form, and checks
        statuses, counters, the device's plan and the pixels of every one."""
        eng = self.engine
        normalize, layout, flip = form
        op = cases[0].op
        assert all(c.op == op for c in cases)
        dirt = self.dirty()
        before = eng.counters()
        out, st = eng.decode_resize([case_image(c) for c in cases], (op.out_h, op.out_w), crop_before_resize=op.crop,
                                    filter=op.filter, normalize=normalize, layout=layout, flip=[flip] * len(cases))
        descs, _ = gpu_debug.snapshot(eng, len(cases))
        after = eng.counters()
        assert (st == 0).all(), st
        assert after["fallback"] == before["fallback"]
        assert after["images"] - before["images"] == len(cases) and after["ok"] - before["ok"] == len(cases)
        assert all(after[k] == before[k] for k in OK_COUNTERS), (before, after)
        assert sum(d.need for d in descs) < dirt, "the noise batch must need more scratch than the cases"
        got = out.cpu().numpy()
        assert got.dtype == (np.float32 if normalize else np.uint8)
        for k, (c, d) in enumerate(zip(cases, descs)):
            check_plan(d, c)
            np.testing.assert_array_equal(got[k], self.ref(c, form), err_msg=f"{c.name} (image {k} of {len(cases)}) {form}")


def check_plan(d, case: Case):
    p = case.plan()
    assert d.status == 0, case.name
    assert (d.width, d.height, d.ncomp) == (case.w, case.h, 1 if case.samp == "gray" else 3), case.name
    got = {f: getattr(d, f) for f in PLAN_FIELDS}
    want = {f: getattr(p, f) for f in PLAN_FIELDS}
    assert got == want, f"{case.name}: the device planned {got}, the restatement {want}"
    route = P.resample_route(d.geo, d.fused, d.rs_fast, d.rs_lay, d.need_h, d.ksh)
    assert P.ROUTE_NAMES[route] == case.route, f"{case.name}: device route {P.ROUTE_NAMES[route]}, intended {case.route}"
    assert (d.fused and -(-case.res[1] // d.tile_w) > 1) == case.multi, case.name


@pytest.fixture(scope="module")
def rig():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Rig()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_alone(rig, case):
    for form in FORMS:
        rig.run([case], form)


def _fillers(op: P.Op) -> list[Case]:
    out = []
    for samp, w, h in STRIP_IMAGES:
        c = Case(f"filler_{samp}_{w}x{h}", w, h, samp, (op.out_h, op.out_w), "", filter=op.filter, crop=op.crop)
        out.append(Case(c.name, w, h, samp, c.res, c.plan().route_name, filter=op.filter, crop=op.crop,
                        multi=c.plan().multi_tile))
    return out


def _mixed_batch(op: P.Op) -> list[Case]:
    """The op's cases spread through tiny filler images of every sampling: more than 32 images."""
    own = [c for c in CASES if c.op == op]
    fill = _fillers(op)
    nf = max(40 - len(own), 12)
    batch = [fill[k % len(fill)] for k in range(nf)]
    for k, c in enumerate(own):
        batch.insert(min(len(batch), 2 + 3 * k), c)
    return batch


OPS = sorted({c.op for c in CASES}, key=lambda o: (o.out_h, o.out_w, o.crop, o.filter))


@pytest.mark.parametrize("op", OPS, ids=lambda o: f"{o.out_h}x{o.out_w}_{o.filter}_{'crop' if o.crop else 'nocrop'}")
def test_cases_in_a_mixed_batch(rig, op):
    batch = _mixed_batch(op)
    assert len(batch) > 32 and all(c in batch for c in CASES if c.op == op)
    for form in FORMS:
        rig.run(batch, form)


@pytest.mark.parametrize("res,filt", STRIP_OPS, ids=[f"{r[0]}x{r[1]}_{f}" for r, f in STRIP_OPS])
def test_64_row_strips(rig, res, filt):
    """A lane of 512 images takes 64-row strips (launch_resample): out_h 65 and 130 are two and three
    strips with a partial last one, over 4:2:0, 4:2:2, 4:4:4, gray and 4:4:0 images in one batch."""
    cs = [c for c in strip_cases() if c.res == res and c.filter == filt]
    assert len(cs) == len(STRIP_IMAGES)
    batch = [cs[k % len(cs)] for k in range(STRIP_BATCH)]
    rig.engine.set_lanes(1)  # one lane of 512: with 4 lanes each would hold 128 images and take 16-row strips
    try:
        assert P.strip_h(len(batch), lanes=1) == [P.K_MAX_STRIP]
        for form in FORMS:
            rig.run(batch, form)
    finally:
        rig.engine.set_lanes(4)
