"""bench.py's plain run, ``--dump-outputs`` and ``--full``: what a dump holds and how a larger
path array is sampled (CPU, a stand-in ensemble), and on the GPU that a plain run reports the
headline only, that two runs with the same arguments dump identical arrays, and that ``--full``
still reports every measurement beside the headline."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"roofline", "repeats", "separate_calls", "cpu_baseline", "accept_kernel_avg_us",
             "rank_diagnostics"}


class _Ensemble:
    """The two read-backs dump_outputs uses, over fixed arrays."""

    def __init__(self, B, P, d):
        rng = np.random.default_rng(7)
        self.X = rng.standard_normal((P, d))
        self.ll = rng.standard_normal(B)
        self.llp = rng.standard_normal(B)

    def get_block_state(self, layout, what, b0, b1):
        from diffusionmcmctools_amd import _lib as L
        return {L.BLK_LL: self.ll, L.BLK_LLPROP: self.llp}[what][b0:b1].copy()

    def download_paths(self, unit, what):
        assert (unit, what) == (0, 0)
        return self.X.copy()


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_holds_the_callers_arrays_as_float64(dmt, tmp_path):
    import bench
    e = _Ensemble(B=6, P=66, d=2)
    res = np.arange(12.0).reshape(4, 3)
    bench.dump_outputs(str(tmp_path / "o"), e, 0, 6, res)
    got = _load(tmp_path / "o")
    assert sorted(got) == ["ll", "ll_prop", "mcmc_run", "paths"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["mcmc_run"], res) and np.array_equal(got["paths"], e.X)
    assert np.array_equal(got["ll"], e.ll) and np.array_equal(got["ll_prop"], e.llp)


def test_dump_samples_a_large_path_array_the_same_way_every_time(dmt, tmp_path, monkeypatch):
    import bench
    assert bench.DUMP_PATH_BYTES <= 48 << 20  # leaves room below 64 MB for the other arrays
    monkeypatch.setattr(bench, "DUMP_PATH_BYTES", 8 * 4 * 100)  # 100 rows of d = 3 and their ids
    e = _Ensemble(B=5, P=1001, d=3)
    res = np.zeros((2, 3))
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), e, 0, 5, res)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["ll", "ll_prop", "mcmc_run", "paths", "paths_rows"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["paths_rows"].astype(np.int64)
    assert rows.shape == (100,) and np.all(np.diff(rows) > 0) and 0 <= rows[0] and rows[-1] < 1001
    assert np.array_equal(a["paths"], e.X[rows])
    assert a["paths"].nbytes + a["paths_rows"].nbytes <= 8 * 4 * 100


def _bench(*args):
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + list(args), capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_reproducibly(tmp_path):
    from diffusionmcmctools_amd import workloads as W
    w = W.c2_ou2d()
    lines = [_bench("--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / n))
             for n in ("a", "b")]
    for line in lines:
        assert HEADLINE <= set(line) and not FULL_ONLY & set(line)
        assert line["steps"] == 3 and line["warmup"] == 2 and line["higher_is_better"] is True
        assert line["unit"] == "steps/s" and line["dtype"] == "f64" and line["ms_per_step"] > 0
        # value and ms_per_step describe the same three timed steps
        assert line["value"] == pytest.approx(w.steps_per_iter / (line["ms_per_step"] * 1e-3),
                                              rel=1e-9)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(b) == ["ll", "ll_prop", "mcmc_run", "paths"]
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k]), k
    assert a["mcmc_run"].shape == (3, 3) and a["ll"].shape == (w.nblocks,)
    assert a["paths"].shape == (sum(sum(r) for r in w.n_points), w.d)
    assert np.all(np.isfinite(a["paths"])) and np.all(np.isfinite(a["ll"]))
    # the timed call's own return value: fetch_ll of the last step is the sum of the blocks' ll,
    # and the accepted counts are the line's accept rate
    assert a["mcmc_run"][-1, 0] == pytest.approx(a["ll"].sum(), rel=1e-12)
    assert lines[0]["accept_rate"] == a["mcmc_run"][:, 2].sum() / (w.nblocks * 3)
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 20


@pytest.mark.gpu
def test_full_run_keeps_every_measurement_beside_the_headline():
    line = _bench("--steps", "3", "--warmup", "2", "--full", "--repeats", "1", "--calls-iters", "5",
                  "--cpu-budget", "0.5")
    assert HEADLINE <= set(line) and FULL_ONLY <= set(line)
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["roofline"]["kernel_avg_us"] > 0 and line["roofline"]["kernel"].startswith("k_")
    assert line["repeats"]["n"] == 1 and line["repeats"]["ms_per_step_median"] > 0
    assert line["separate_calls"]["iterations"] == 5
    assert line["cpu_baseline"]["value"] > 0
    assert line["decisions_total"] > 0 and line["decisions_identical"] == line["decisions_total"]
