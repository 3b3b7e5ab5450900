"""bench.py's plain run and --dump-outputs: the plain line carries the headline keys and none of
--full's legs; the dumped arrays are float32, finite, within the size budget and identical between
two runs with different step counts (seeded inputs and weights); the sampling helper is seeded."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("eager_value", "roofline", "latency_b1", "cpu_baseline", "parity", "fp32_value", "host_feed", "api")


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sampled_is_seeded_and_zeroes_unwritten(bench):
    n = bench.DUMP_SAMPLE
    t = torch.arange(4 * n, dtype=torch.float32).reshape(4, n)
    a, b = bench.sampled(t, 5), bench.sampled(t, 5)
    assert a.dtype == np.float32 and a.shape == (n,) and np.array_equal(a, b)
    assert not np.array_equal(a, bench.sampled(t, 6))
    # a transposed view samples the same logical elements as its contiguous copy
    assert np.array_equal(bench.sampled(t.t(), 5), bench.sampled(t.t().contiguous(), 5))
    rows = torch.tensor([True, False, True, False])[:, None]
    m = bench.sampled(t + 1.0, 5, rows)
    assert np.array_equal(m != 0, (a.astype(np.int64) // n) % 2 == 0)
    small = torch.ones(3, 4, 2)
    s = bench.sampled(small, 1, torch.arange(4)[None, :, None] < torch.tensor([0, 2, 4])[:, None, None])
    assert s.shape == (3, 4, 2) and s.sum(axis=(1, 2)).tolist() == [0.0, 4.0, 8.0]


def test_dump_arrays_writes_float32(bench, tmp_path):
    bench.dump_arrays(str(tmp_path / "d"), {"x": np.arange(6, dtype=np.float64).reshape(2, 3)})
    x = np.load(tmp_path / "d" / "x.npy")
    assert x.dtype == np.float32 and x.shape == (2, 3) and x[1, 2] == 5.0


def test_zero_steps_refused():
    r = subprocess.run([sys.executable, BENCH, "--cpu-dryrun", "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


def run_plain(*runs):
    """(steps, warmup, dump directory) per run; the runs are separate processes, started together."""
    procs = [subprocess.Popen([sys.executable, BENCH, "--gpus", "1", "--batch", "8", "--steps", str(steps),
                               "--warmup", str(warmup), "--dump-outputs", str(out)], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for steps, warmup, out in runs]
    try:
        outs = [p.communicate(timeout=120) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    res = []
    for p, (stdout, stderr) in zip(procs, outs):
        assert p.returncode == 0, stderr[-2000:]
        lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        res.append(json.loads(lines[0]))
    return res


@pytest.mark.gpu
def test_plain_run_line_and_dump_repeat(tmp_path):
    a, b = run_plain((3, 1, tmp_path / "a"), (2, 0, tmp_path / "b"))
    for line, steps in ((a, 3), (b, 2)):
        assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
        assert line["steps"] == steps and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(8 * 1e3 / line["ms_per_step"], rel=1e-3)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"records.npy", "counts.npy", "head_heatmap.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert 0 < total <= 64 * 2 ** 20
    rec, cnt = np.load(tmp_path / "a" / "records.npy"), np.load(tmp_path / "a" / "counts.npy")
    assert rec.shape == (8, 100, 10) and cnt.shape == (8,) and cnt.max() > 0
    for f in range(8):  # rows past a frame's count are dumped as 0, the ones before hold a score
        k = int(cnt[f])
        assert not rec[f, k:].any() and (rec[f, :k, 1] > 0).all()
