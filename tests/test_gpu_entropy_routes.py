"""Every entropy / unstuff plan edge on the GPU, stage by stage against the oracle.

The cases come from tests/entropy_cases.py; tests/test_entropy_cases_table.py proves on the CPU that they hold
every situation (group counts on either side of each threshold and at the kMaxEntGroups cap, groups with an
empty share, more sync tasks than a round takes, restart segments beginning at a chunk boundary of the segmented
scan, nseg > 256, subsequences of many and of fewer than two block boundaries, the 10-bit route multi-group and
with restart intervals, the multi-hypothesis pass on and off, FF|00 / FF|Dn / FF FF|Dn across thread and tile
boundaries in both unstuff routes, 64 | 65 tiles, the scan's start at every residue mod 16).  Every case runs in
both modes -- alone (a chunk of one image: the latency plan) and at index 17 of a chunk of 40
(the throughput plan) -- and for each run

  * status 0, the engine's counters, `fallback` unchanged;
  * the descriptor's plan fields equal what the real plan_sample printed for that case and mode on the CPU
    (test_entropy_cases_table.plan_table; warm_bits is the small lane's, which k_parse sets), so the edge is
    reached, not only planned; nsub, ulen, useg_found and the run-time conditions of the case's situations
    (sync_rounds, pad0) hold; the subsequences at which the device begins a restart segment (SubState::first at
    off_sub) are those of the restated layout -- 63, 64 and 65 for the three chunk-boundary cases;
  * stage 1: per restart segment the bytes at off_ustream[lo, hi) equal the restated unstuffing's;
  * stage 2: the coefficient blocks (tests/coef_compact.py, whichever format the mode uses) equal the oracle's,
    every block of every case (the cap cases too: the full read-back takes well under a second);
  * pixels equal ``O.pipeline`` bit for bit at 48 x 64 with the crop, and ``O.decode`` at the image's own size
    (layout "hwc", the same-size shortcut) for cases under 1 MP.

Dirtied scratch: before every decode the same engine decodes a batch of noise JPEGs whose scratch need is larger
(asserted), so subsequence states, records, tile tables and coefficient slots hold stale non-zero bytes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)
from tests import entropy_cases as E  # noqa: E402
from tests import gpu_debug  # noqa: E402
from tests.coef_compact import blocks_differing_from_oracle, is_compact, read_blocks  # noqa: E402
from tests.entropy_cases import BATCH, CASES, SITUATIONS, Case, case_image  # noqa: E402
from tests.resample_cases import STRIP_IMAGES, image as filler_image  # noqa: E402
from tests.test_entropy_cases_table import plan_table, unstuff  # noqa: E402
from tests.test_plan_host import build_driver  # noqa: E402

RES = (48, 64)
AT = 17  # the case's place in its chunk of BATCH
PLAN_FIELDS = ("entropy_len", "nseg", "ntiles", "sub_bits", "nsub_cap", "ent_groups", "lat", "mh")
OK_COUNTERS = ("unsupported", "corrupt", "capacity", "other")


class Rig:
    def __init__(self):
        from sds_amd.engine import JpegEngine
        from tests.golden.synth import encode_jpeg
        self.engine = JpegEngine(max_batch=256)
        rng = np.random.default_rng(2024)
        noise = [encode_jpeg(rng.integers(0, 256, (480, 640, 3), dtype=np.uint8), 95) for _ in range(4)]
        self.noise = [noise[k % 4] for k in range(24)]
        self.fillers = [filler_image(*STRIP_IMAGES[k % len(STRIP_IMAGES)]) for k in range(BATCH - 1)]
        self.refs = {}

    def dirty(self) -> int:
        """Decodes the noise batch; returns the scratch bytes it took (the next decode must take fewer)."""
        _, st = self.engine.decode_resize(self.noise, (32, 32))
        assert (st == 0).all()
        descs, _ = gpu_debug.snapshot(self.engine, len(self.noise))
        return sum(d.need for d in descs)

    def ref(self, jpg: bytes, what: str) -> np.ndarray:
        """The oracle's small output ("small") or full decode ("full") of a file, computed once."""
        key = (jpg, what)
        if key not in self.refs:
            r = O.pipeline(jpg, RES) if what == "small" else O.decode(jpg)
            r.setflags(write=False)
            self.refs[key] = r
        return self.refs[key]

    def chunk(self, jpgs, mode):
        """(files, indices of jpgs in them): jpgs as they are, or from index AT of a chunk of BATCH."""
        if mode == "alone":
            assert len(jpgs) <= E.const("kSmallBatch")
            return list(jpgs), list(range(len(jpgs)))
        assert BATCH > E.const("kSmallBatch")
        files = self.fillers[:AT] + list(jpgs) + self.fillers[AT:]
        return files[:max(BATCH, AT + len(jpgs))], list(range(AT, AT + len(jpgs)))

    def decode(self, files, res, **kw):
        """Dirties the scratch, decodes one chunk; checks statuses and counters.  (out, descs, fetch)"""
        eng = self.engine
        dirt = self.dirty()
        before = eng.counters()
        out, st = eng.decode_resize(files, res, **kw)
        descs, fetch = gpu_debug.snapshot(eng, len(files))
        after = eng.counters()
        assert (st == 0).all(), st
        assert after["fallback"] == before["fallback"]
        assert after["images"] - before["images"] == len(files) and after["ok"] - before["ok"] == len(files)
        assert all(after[k] == before[k] for k in OK_COUNTERS), (before, after)
        assert sum(d.need for d in descs) < dirt, "the noise batch must need more scratch than the cases"
        return out, descs, fetch


@pytest.fixture(scope="module")
def plans():
    """The plan driver's rows for every case and mode, from a plain build of the driver: the sanitized build and
    run belong to tests/test_entropy_cases_table.py, on the CPU.  Without a compiler this fails: the net must
    not go quiet for a reason that is not the hardware."""
    import shutil
    assert shutil.which("g++"), "tests/asan/plan_driver.cpp must be built for the expected plans: no g++"
    return plan_table(build_driver(sanitize=False))


@pytest.fixture(scope="module")
def rig():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Rig()


def check_case(rig, p: dict, case: Case, mode: str, jpg: bytes, d, fetch, got: np.ndarray):
    what = f"{case.name} [{mode}]"
    # -- the plan, as the CPU driver printed it, and the run-time properties
    dev = {f: getattr(d, f) for f in PLAN_FIELDS}
    assert dev == {f: p[f] for f in PLAN_FIELDS}, f"{what}: the device planned {dev}"
    assert d.warm_bits == p["warm_small"], what  # a lane of fewer than kWarmSmallLane images (or the latency plan)
    assert d.entropy_off == E.entropy_off(jpg) and d.status == 0, what
    run_time = {"nsub": d.nsub, "ulen": d.ulen, "useg": d.useg_found}
    assert run_time == {f: p[f] for f in run_time}, f"{what}: the device found {run_time}"
    now = dict(p, sync_rounds=d.sync_rounds, pad0=d.pad0)
    print(f"{what}: ent_groups {d.ent_groups} sub_bits {d.sub_bits} nsub {d.nsub} sync_rounds {d.sync_rounds} "
          f"pad0 {d.pad0} ntiles {d.ntiles} warm_bits {d.warm_bits} mh {d.mh} nseg {d.nseg}")
    for s in case.pins:
        if SITUATIONS[s][0] == mode:
            E.check(now, SITUATIONS[s][1], runtime=True, what=f"{what} {s}")
    # -- the subsequence layout the device built: where each restart segment begins (SubState::first, ::seg)
    if not d.mh:  # (the multi-hypothesis pass lays its one segment out itself: mh_layout)
        sub = gpu_debug.sub_states(d, fetch)
        first = {int(j) for j in np.flatnonzero(sub["first"])}
        assert first == {j for j in p["first_at"] if j < d.nsub}, f"{what}: segments begin at {sorted(first)[:70]}"
        assert (np.diff(sub["seg"]) == sub["first"][1:]).all() and sub["seg"][0] == 0, what
    # -- stage 1: the unstuffed stream, per restart segment
    segs, end = unstuff(jpg)
    assert end == 0xD9 and len(segs) == d.nseg
    table = fetch(d.off_seg, (2 * d.nseg + 2) * 4).view(np.int32)
    lo, hi = table[:d.nseg], table[d.nseg + 1:2 * d.nseg + 1]  # seg_view: lo [nseg + 1], then hi
    stream = fetch(d.off_ustream, int(d.ulen)).tobytes()
    at = 0
    for k, s in enumerate(segs):
        assert (int(lo[k]), int(hi[k])) == (at, at + len(s)), f"{what}: segment {k} of {len(segs)}"
        at += len(s)
    assert stream == b"".join(segs), f"{what}: unstuffed bytes"
    # -- stage 2: every coefficient block
    assert is_compact(d) == (mode == "batch" and p["ent"] != "kRtEnt10"), what
    zz, _ = read_blocks(d, fetch)
    assert blocks_differing_from_oracle(d, zz, jpg) == [0] * d.ncomp, what
    # -- pixels
    np.testing.assert_array_equal(got, rig.ref(jpg, "small"), err_msg=what)


def run_cases(rig, plans, cases, mode):
    jpgs = [case_image(c) for c in cases]
    files, idx = rig.chunk(jpgs, mode)
    out, descs, fetch = rig.decode(files, RES)
    got = out.cpu().numpy()
    for c, j, k in zip(cases, jpgs, idx):
        check_case(rig, plans[c.name, mode], c, mode, j, descs[k], fetch, got[k])


SINGLE = [c for c in CASES if c.group != "residue"]
RESIDUES = [c for c in CASES if c.group == "residue"]


@pytest.mark.parametrize("mode", ["alone", "batch"])
@pytest.mark.parametrize("case", SINGLE, ids=lambda c: c.name)
def test_case(rig, plans, case, mode):
    """Every case in both modes: the situations it pins name one of them or both, the other runs all the same."""
    run_cases(rig, plans, [case], mode)
    if case.big:
        return
    jpg = case_image(case)
    full = rig.ref(jpg, "full")
    files, idx = rig.chunk([jpg], mode)
    out, descs, _ = rig.decode(files, full.shape[:2], layout="hwc")
    assert descs[idx[0]].geo == 1  # kGeoIdentity: the same-size shortcut
    np.testing.assert_array_equal(out[idx[0]].cpu().numpy(), full, err_msg=f"{case.name} [{mode}] full size")


@pytest.mark.parametrize("mode", ["alone", "batch"])
def test_scan_start_at_every_residue(rig, plans, mode):
    """The 16 copies of one small image whose scans start at file offsets of every residue mod 16, in one chunk."""
    assert len(RESIDUES) == 16
    run_cases(rig, plans, RESIDUES, mode)


def test_scan_start_at_every_residue_of_a_device_blob(rig):
    """Through the device-resident entry point (always the throughput plan: k_us_serial for these), each of the
    16 copies at blob offsets of every residue mod 16: 256 samples, the scan's first byte at every alignment
    from both causes."""
    jpgs = [case_image(c) for c in RESIDUES]
    parts, offs, lens, which, pos = [], [], [], [], 0
    for shift in range(16):
        for k, j in enumerate(jpgs):
            gap = (shift - pos) % 16
            parts.append(bytes(gap) + j)
            pos += gap
            offs.append(pos)
            lens.append(len(j))
            which.append(k)
            pos += len(j)
    assert {(o % 16, (o + E.entropy_off(jpgs[k])) % 16) for o, k in zip(offs, which)} == {(a, b) for a in range(16) for b in range(16)}
    blob = torch.from_numpy(np.frombuffer(b"".join(parts), np.uint8).copy()).cuda()
    rig.dirty()
    out, st = rig.engine.decode_resize_device(blob, torch.tensor(offs, dtype=torch.int64).cuda(),
                                              torch.tensor(lens, dtype=torch.int32).cuda(), RES)
    assert (st.cpu() == 0).all()
    descs, _ = gpu_debug.snapshot(rig.engine, len(offs))
    assert all(d.lat == 0 and 0 < d.ntiles <= E.const("kUsSerialTiles") for d in descs)
    got = out.cpu().numpy()
    for i, k in enumerate(which):
        np.testing.assert_array_equal(got[i], rig.ref(jpgs[k], "small"), err_msg=f"sample {i}: copy {k} at {offs[i]}")


def _oracle_result(jpg):
    try:
        return O.OK, O.pipeline(jpg, RES)
    except O.OracleError as e:
        return e.status, None


TRUNCATED = [c for c in CASES if c.truncate]


@pytest.mark.parametrize("mode", ["alone", "batch"])
@pytest.mark.parametrize("case", TRUNCATED, ids=lambda c: c.name)
def test_truncated_copies(rig, case, mode):
    """A copy cut at 2/3 of the file between two whole ones: status and pixels equal the oracle's (as
    test_gpu_parity.test_tile_parallel_unstuff_vs_oracle), for a multi-group case, the empty-share case and the
    sync-pressure case."""
    jpg = case_image(case)
    three = [jpg, jpg[:len(jpg) * 2 // 3], jpg]
    files, idx = rig.chunk(three, mode)
    rig.dirty()
    got, st = rig.engine.decode_resize(files, RES)
    for k, j in zip(idx, three):
        ost, ref = _oracle_result(j)
        assert int(st[k]) == ost, f"{case.name} [{mode}] sample {k}: gpu {int(st[k])} vs oracle {ost}"
        if ost == O.OK:
            np.testing.assert_array_equal(got[k].cpu().numpy(), ref, err_msg=f"{case.name} [{mode}] sample {k}")
