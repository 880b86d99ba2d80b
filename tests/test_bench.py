"""bench.py's own options: --dump-outputs writes what the last timed step computed, --steps sets the timed steps, a plain
run prints the headline and nothing that needs runs of its own, --full adds the rest."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

SMALL = ["--views", "20000", "--edges", "300000"]


def _line(r):
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(lines[0])


def test_dump_outputs_below_the_limit_writes_everything(tmp_path):
    rng = np.random.default_rng(3)
    arrays = {"rotations": np.asfortranarray(rng.normal(size=(50, 4))), "weights": rng.random(200),
              "scores": np.arange(5, dtype=np.float64)}
    shapes = bench.dump_outputs(str(tmp_path), arrays)
    assert shapes == {"rotations": [50, 4], "weights": [200], "scores": [5]}
    for name, a in arrays.items():
        b = np.load(tmp_path / (name + ".npy"))
        assert b.dtype == np.float64 and np.array_equal(b, a)
    assert not list(tmp_path.glob("*_rows.npy"))


def test_dump_outputs_above_the_limit_writes_a_fixed_sample(tmp_path):
    rng = np.random.default_rng(4)
    arrays = {"rotations": rng.normal(size=(40000, 4)), "weights": rng.random(100000)}
    limit = 1 << 20
    bench.dump_outputs(str(tmp_path / "a"), arrays, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), arrays, limit=limit)
    total = sum(f.stat().st_size for f in (tmp_path / "a").iterdir())
    assert total <= limit
    for name, a in arrays.items():
        rows = np.load(tmp_path / "a" / (name + "_rows.npy"))
        got = np.load(tmp_path / "a" / (name + ".npy"))
        assert rows.dtype == np.float64 and 0.1 * len(a) < len(rows) < len(a)
        assert np.all(np.diff(rows) > 0)
        assert np.array_equal(got, a[rows.astype(np.int64)])
        # the same arguments give the same sample
        assert np.array_equal(rows, np.load(tmp_path / "b" / (name + "_rows.npy")))


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=60, cwd=ROOT)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_help_names_the_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=60, cwd=ROOT)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path):
    """a plain run: the headline fields, exactly --steps timed steps, no roofline or leg; the dumped arrays are what an
    irls of the same graph from the same start returns"""
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(d)] + SMALL, capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = _line(r)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0 and line["dtype"] == "f64"
    assert not any(k.startswith(("roofline", "also_", "cpu_baseline")) for k in line), sorted(line)
    assert line["outputs"]["shapes"] == {"rotations": [20000, 4], "weights": [300000],
                                         "scores": [line["iters_to_converge"]]}
    Q, w, sc = (np.load(d / (n + ".npy")) for n in ("rotations", "weights", "scores"))
    assert Q.dtype == w.dtype == sc.dtype == np.float64
    np.testing.assert_allclose(sc, line["final_scores"], rtol=1e-12)
    from irotavg_amd import capi
    S, Q0 = bench.build_problem(20000, 300000, 0.0, 0)
    with capi.Graph(S["I"], S["QQ"], S["n"], 1, pcg_rtol=1e-10) as G:
        G.set_rotations(Q0)
        res = G.irls(4, bench.SIG, 100, 1e-3)
        Qr, wr = G.get_rotations(), G.get_weights()
    assert res["iters"] == line["iters_to_converge"]
    np.testing.assert_allclose(Q, Qr, rtol=0, atol=1e-12)
    np.testing.assert_allclose(w, wr, rtol=1e-12, atol=1e-15)


@pytest.mark.gpu
def test_full_run_carries_the_rooflines():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--full", "--no-cpu", "--no-pmc"] + SMALL, capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = _line(r)
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert "roofline" in line and "kernels" in line and "roofline_edge_residual" in line
