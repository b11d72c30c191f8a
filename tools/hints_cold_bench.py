"""bench.py's workload with the entry-point store emptied before every step: the cold cost of the store (every
row a miss: the lookup, the speculative and sync passes, the record written) next to bench.py's own steady state,
where every row is a hit.  Same arguments and the same JSON line as bench.py (one GPU).
    python tools/hints_cold_bench.py [bench.py arguments]"""
import os
import runpy
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from sds_amd.engine import JpegEngine  # noqa: E402

_decode = JpegEngine.decode_resize_device


def _cold(self, *a, **kw):
    self.clear_hints()
    return _decode(self, *a, **kw)


JpegEngine.decode_resize_device = _cold
sys.argv = [os.path.join(REPO, "bench.py")] + sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
