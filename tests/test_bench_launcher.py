"""bench.py's multi-rank launcher (configs[3] shape) on CPU: ``--gpus 2`` outside torchrun starts two
fresh rank processes that join a gloo process group, each owning its compute_index_slice rows, and
rank 0 prints one line with the aggregate rate and both per-rank rates.  The engine is the CPU
stand-in (``--engine stub``); the HIP path of the same script runs on the GPU box."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(gpus, *extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--full", "--gpus", str(gpus), "--engine", "stub",
           "--backend", "gloo", "--rows", "64", "--pool", "4", "--batch", "16", "--steps", "3", "--warmup", "1",
           "--no-cpu-baseline", "--roofline-steps", "1", *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout  # only rank 0 prints
    return json.loads(lines[0])


def test_two_rank_launch_reports_the_whole_job():
    line = _run(2)
    assert line["n_gpus"] == 2
    pg = line["process_group"]
    assert (pg["backend"], pg["world_size"], pg["gpus_visible"], pg["all_gather_device"]) == ("gloo", 2, 0, "cpu")
    assert len(line["per_rank_images_per_s"]) == 2
    assert line["config"]["global_batch"] == 32 and line["config"]["rows_per_gpu"] == 64
    # the parquet index the ranks sliced (sds/index.py:208-246): 2 x 64 rows, one contiguous slice each
    assert line["config"]["index"]["rows"] == 128 and "parquet" in line["config"]["index"]["source"]
    assert line["config"]["index"]["slices"] == [[0, 64], [64, 128]]
    # value = all ranks' images over the slowest rank's time
    slowest = min(line["per_rank_images_per_s"])
    assert abs(line["value"] - 2 * slowest) <= 0.01 * line["value"] + 1


def test_one_gpu_run_is_unchanged():
    line = _run(1)
    assert line["n_gpus"] == 1 and line["process_group"]["world_size"] == 1
    assert len(line["per_rank_images_per_s"]) == 1
    assert line["config"]["index"]["slices"] == [[0, 64]]


def test_forced_process_group_at_world_size_1():
    """--force-pg: one rank still creates the process group and runs the collectives of the multi-GPU path
    (the GPU test runs it with nccl = RCCL)."""
    line = _run(1, "--force-pg")
    pg = line["process_group"]
    assert pg["backend"] == "gloo" and pg["world_size"] == 1 and pg["forced_at_world_size_1"]
    assert pg["all_gather_device"] == "cpu"
    assert line["n_gpus"] == 1 and len(line["per_rank_images_per_s"]) == 1


def test_default_index_is_a_million_rows_on_several_gpus():
    """configs[3]: without --rows, --gpus N slices a 1,000,000-row parquet index (125,000 rows per rank at 8)."""
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--full", "--gpus", "2", "--engine", "stub",
           "--backend", "gloo", "--pool", "4", "--batch", "16", "--steps", "1", "--warmup", "0", "--no-cpu-baseline",
           "--roofline-steps", "1"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert line["config"]["index"]["rows"] == 1_000_000 and line["config"]["rows_per_gpu"] == 500_000
    assert line["config"]["index"]["slices"] == [[0, 500_000], [500_000, 1_000_000]]
    assert line["config"]["workload"].startswith("configs[3]: 1,000,000-row parquet index")


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """Without --full the line carries the headline figures only (what --full measures is null), --steps sets
    the number of timed steps, and --dump-outputs writes the last step's outputs as float32 / float64 .npy
    files, the same from run to run."""
    import numpy as np

    def run(d, steps):
        cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--engine", "stub", "--rows", "64",
               "--pool", "4", "--batch", "16", "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(d)]
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        return json.loads(lines[0])

    line = run(tmp_path / "a", 3)
    assert line["full"] is False and line["steps"] == 3
    for k in ("roofline", "stage_ms_per_step_single_lane", "pixel_check", "cpu_baseline"):
        assert line[k] is None, k
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    # value and ms_per_step describe the same timed region: batch x steps images in steps x ms_per_step
    assert line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - 16) <= 0.02 * 16
    assert sorted(os.listdir(tmp_path / "a")) == ["out.npy", "out_rows.npy", "status.npy"]
    assert line["outputs_dumped"]["files"] == ["out.npy", "out_rows.npy", "status.npy"]
    out, rows, st = (np.load(tmp_path / "a" / f"{n}.npy") for n in ("out", "out_rows", "status"))
    assert out.dtype == np.float32 and out.shape == (16, 3, 256, 256) and st.dtype == np.float32 and st.shape == (16,)
    # 1 gate + 1 warm-up + 3 timed batches of 16 rows over 64 resident rows: the last one starts at row 0
    assert rows.dtype == np.float64 and rows.tolist() == list(range(0, 16))
    assert out.nbytes + rows.nbytes + st.nbytes <= 64 * 10 ** 6
    run(tmp_path / "b", 3)
    for n in ("out", "out_rows", "status"):
        np.testing.assert_array_equal(np.load(tmp_path / "b" / f"{n}.npy"), np.load(tmp_path / "a" / f"{n}.npy"))


def test_dump_outputs_samples_a_fixed_set_of_rows_within_the_budget(tmp_path):
    """An output larger than the budget is dumped as a seeded sample of its rows: the same rows on every call, in
    ascending position, their values and row indices side by side; the statuses are written whole."""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    out = torch.arange(40 * 3 * 2 * 2, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(40, 3, 2, 2)
    status = torch.arange(40, dtype=torch.int32) % 3
    ids = (100 + np.arange(40)) % 120
    info = bench.dump_outputs(str(tmp_path / "a"), out, status, ids, 0, 1, budget=7 * 12 * 4 + 5)
    assert info["rows"] == 7 and info["of"] == 40
    got, rows, st = (np.load(tmp_path / "a" / f"{n}.npy") for n in ("out", "out_rows", "status"))
    assert got.dtype == np.float32 and got.shape == (7, 3, 2, 2) and rows.dtype == np.float64
    pos = [int(np.flatnonzero(ids == r)[0]) for r in rows]
    assert pos == sorted(set(pos)) and len(pos) == 7
    np.testing.assert_array_equal(got, out.numpy()[pos].astype(np.float32))
    np.testing.assert_array_equal(st, status.numpy().astype(np.float32))
    bench.dump_outputs(str(tmp_path / "b"), out, status, ids, 0, 1, budget=7 * 12 * 4 + 5)
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "out_rows.npy"), rows)
    # an order (configs[4]: the batch in completion order) puts the batch in row-index order before sampling
    perm = np.random.default_rng(3).permutation(40)
    bench.dump_outputs(str(tmp_path / "c"), out[perm], status[perm], ids[perm], 0, 1, order=np.argsort(perm),
                       budget=7 * 12 * 4 + 5)
    for n, want in (("out", got), ("out_rows", rows), ("status", st)):
        np.testing.assert_array_equal(np.load(tmp_path / "c" / f"{n}.npy"), want)
