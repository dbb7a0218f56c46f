"""Posterior path moments (include/dmt.h, "posterior path moments") without a GPU: the host
entry point dmt_moments_rule against the NumPy restatement of tests/_moments_ref.py bit for bit,
Welford's update against np.mean / np.var, argument checks, the high-level API on the oracle
engine, and the seed check of the GPU cases (tests/test_path_moments_gpu.py) on their oracle
twins."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import diffusionmcmctools_amd as dmt
from diffusionmcmctools_amd import _lib as L
from diffusionmcmctools_amd import engine as E

import _moments_ref as mr

N_ELEM, N_SAMPLES = 1000, 40


def _samples(seed=3, as_f32=False):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N_SAMPLES, N_ELEM)) * rng.uniform(0.1, 30.0, N_ELEM) \
        + rng.uniform(-50.0, 50.0, N_ELEM)
    return x.astype(np.float32).astype(np.float64) if as_f32 else x


def _host_fold(samples, alias):
    mean, m2 = np.zeros(samples.shape[1]), np.zeros(samples.shape[1])
    for k, x in enumerate(samples, 1):
        if alias:
            E.moments_rule(x, mean, m2, k, out=(mean, m2))
        else:
            mean, m2 = E.moments_rule(x, mean, m2, k)
    return mean, m2


@pytest.mark.parametrize("as_f32", [False, True], ids=["f64", "f32_values"])
@pytest.mark.parametrize("alias", [False, True], ids=["separate", "aliased"])
def test_host_rule_equals_numpy_fold_bit_for_bit(as_f32, alias):
    x = _samples(as_f32=as_f32)
    mean, m2 = _host_fold(x, alias)
    rm, rs, n = mr.fold(x)
    assert n == N_SAMPLES
    assert np.array_equal(mr.bits(mean), mr.bits(rm))
    assert np.array_equal(mr.bits(m2), mr.bits(rs))


def test_count_one_from_zeros():
    x = _samples()[0]
    mean, m2 = E.moments_rule(x, np.zeros(N_ELEM), np.zeros(N_ELEM), 1)
    rm, rs = mr.rule(x, np.zeros(N_ELEM), np.zeros(N_ELEM), 1)
    assert np.array_equal(mr.bits(mean), mr.bits(rm)) and np.array_equal(mr.bits(m2), mr.bits(rs))
    assert np.array_equal(mean, x)          # 0 + (x − 0) / 1
    assert np.array_equal(m2, np.zeros(N_ELEM))  # delta · (x − x)


def test_welford_agrees_with_mean_and_variance():
    """|mean − np.mean| <= 8·eps·max|x| and |m2 − (n−1)·np.var(ddof=1)| <= 8·eps·n·max|x|²: each
    of the n steps adds a relative rounding error of a few eps to quantities bounded by max|x|
    (mean) and n·max|x|² (m2); the bounds follow from the recurrence, they are not tuned."""
    x = _samples()
    mean, m2 = _host_fold(x, alias=False)
    n, eps, mx = N_SAMPLES, np.finfo(np.float64).eps, np.abs(x).max()
    assert np.abs(mean - np.mean(x, axis=0)).max() <= 8 * eps * mx
    assert np.abs(m2 - np.var(x, axis=0, ddof=1) * (n - 1)).max() <= 8 * eps * n * mx * mx


@pytest.mark.parametrize("n,count", [(-1, 1), (4, 0), (4, -3)])
def test_rule_rejects_bad_arguments(n, count):
    a = np.zeros(4)
    st = L.lib.dmt_moments_rule(n, count, L.f64p(a), L.f64p(a), L.f64p(a), L.f64p(a), L.f64p(a))
    assert st == L.ERR_INVALID


def test_rule_rejects_null_arrays():
    a = np.zeros(4)
    assert L.lib.dmt_moments_rule(4, 1, None, L.f64p(a), L.f64p(a), L.f64p(a), L.f64p(a)) == L.ERR_INVALID
    assert L.lib.dmt_moments_rule(4, 1, L.f64p(a), L.f64p(a), L.f64p(a), None, L.f64p(a)) == L.ERR_INVALID
    assert L.lib.dmt_moments_rule(0, 1, None, None, None, None, None) == L.OK


def test_timing_class_and_symbols():
    assert L.K_MOMENTS == 5
    for name in ("dmt_moments_reserve", "dmt_moments_reset", "dmt_moments_accumulate",
                 "dmt_set_run_moments", "dmt_moments_state", "dmt_moments_download",
                 "dmt_moments_upload", "dmt_moments_rule"):
        assert name in L.SYMBOLS and hasattr(L.lib, name)
    src = open(L.INCLUDE_H).read()
    assert "DMT_K_MOMENTS = 5" in src and "DMT_K_COUNT = 6" in src


def test_kernels_use_no_scratch():
    """Every instantiation of the three k_path_moments kernels (wave, rows, packets) keeps its
    state in registers: no spill, no scratch (the build's resource-usage remarks, as
    tests/test_resource_usage.py reads them)."""
    from test_resource_usage import load_usage
    mine = {k: v for k, v in load_usage().items() if "dmt::k_path_moments_" in k}
    assert len(mine) == 11, sorted(mine)  # wave × 2 precisions, rows × 2 × d = 1..3, pk × d = 1..3
    for name, u in mine.items():
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["Occupancy"] >= 4, (name, u)


# ------------------------------------------------------------------ seeds of the GPU cases
_TWIN = {}


def _twin_run(case, n=10):
    """The oracle twin of GPU test 1: n one-iteration runs, XX downloaded after each."""
    if case not in _TWIN:
        _, ora, plan = mr.build(case, device=False)
        xs = []
        for i in range(1, n + 1):
            mr.step(ora, plan, i, case in mr.RAGGED)
            xs.append(ora.download_paths(L.U, 0).copy())
        _TWIN[case] = (ora, plan, xs)
    return _TWIN[case]


@pytest.mark.parametrize("case", mr.CASES)
def test_seeds_of_the_gpu_cases_on_the_oracle_twin(case):
    ora, plan, xs = _twin_run(case)
    mr.check_seed_condition(ora, case, plan, list(range(1, 11)))
    assert any(not np.array_equal(xs[0], x) for x in xs[1:])


# ------------------------------------------------------------------ high-level API on the oracle
def _api_on_oracle():
    import oracle as orc
    case = "fhn_wave"
    _, ora, plan = mr.build(case, device=False)
    data = mr.cs.ragged_case()
    se = dmt.SamplingEnsemble(data["model"], data["n_points"], _engine=ora)
    return se, ora, plan


def test_api_path_moments_on_the_oracle_engine():
    se, ora, plan = _api_on_oracle()
    with pytest.raises(RuntimeError):
        se.accumulate_path_moments(1)
    se.reserve_path_moments()
    xs = []
    for i in range(1, 7):
        mr.step(ora, plan, i, True)
        se.accumulate_path_moments(i)
        xs.append(ora.download_paths(L.U, 0).copy())
    mean, var, n = se.path_moments()
    rm, rs, rn = mr.fold(xs)
    assert n == rn == 6
    assert len(mean) == 3 and [len(r) for r in mean] == [4, 6, 5]
    assert np.array_equal(mr.bits(np.concatenate([s for r in mean for s in r])), mr.bits(rm))
    assert np.array_equal(mr.bits(np.concatenate([s for r in var for s in r])), mr.bits(rs / 5))
    se.reserve_path_moments()  # zeroes
    with pytest.raises(ValueError):
        se.path_moments()
    se.accumulate_path_moments(7)
    with pytest.raises(ValueError):
        se.path_moments()      # one sample: no variance
    m1, v1, n1 = se.path_moments(var=False)
    assert n1 == 1 and v1 is None


def test_api_path_moments_every_on_the_oracle_engine():
    """path_moments_every on an engine without device moments cuts mcmc_run as the device does:
    the same out as the unsplit run, moments of iterations 6, 9, 12 (every 3, burn-in 5)."""
    se, ora, plan = _api_on_oracle()
    se2, ora2, _ = _api_on_oracle()
    lay, nb = plan[0]
    be = _block_ensemble(se, lay, nb)
    be2 = _block_ensemble(se2, lay, nb)
    se.reserve_path_moments()
    se.path_moments_every(3, burn_in=5)
    out = be.mcmc_run(2, 12, salt=0)
    xs, outs = [], []
    for it, n in ((2, 5), (7, 3), (10, 3), (13, 1)):
        outs.append(be2.mcmc_run(it, n, salt=0))
        if (it + n - 1) % 3 == 0:
            xs.append(ora2.download_paths(L.U, 0).copy())
    assert np.array_equal(out, np.concatenate(outs))
    mean, var, n = se.path_moments()
    rm, rs, rn = mr.fold(xs)
    assert n == rn == 3
    assert np.array_equal(mr.bits(np.concatenate([s for r in mean for s in r])), mr.bits(rm))


def _block_ensemble(se, lay, nb):
    """A BlockEnsemble view of an existing layout of the engine (the test seam's shortcut)."""
    from diffusionmcmctools_amd.api import _BlockRange
    br = _BlockRange(se.ens, lay, 0, nb, mr.HIST)
    br._global = False
    return br


def test_smoothing_example_on_the_oracle_backend():
    """examples/fhn_smoothing.py: the estimate equals the fold of the paths a caller would have
    kept (every 4th iteration after a burn-in of 10), formed here from the same run on a twin."""
    import os
    import sys
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import fhn_smoothing as fs
    import reference_tutorials as T
    from diffusionmcmctools_amd.api import engine_override
    from diffusionmcmctools_amd.models import FitzHughNagumoAux
    import oracle as orc

    def factory(model, n_points, prec, seed):
        return orc.OracleEnsemble(model.kind, model.d, model.m, n_points, prec=prec, seed=seed)
    rec = T.preamble_recordings()
    with engine_override(factory):
        mean, std, n, st = fs.smoothing_estimate(FitzHughNagumoAux, rec, 0.01, ρ=0.9,
                                                 num_steps=30, burn_in=10, every=4)
        _, _, _, st2 = fs.smoothing_estimate(FitzHughNagumoAux, rec, 0.01, ρ=0.9, num_steps=30,
                                             burn_in=10, every=0)
    assert n == 5  # iterations 12, 16, 20, 24, 28
    assert len(mean) == len(rec.obs) and all(m.shape == s.shape for m, s in zip(mean, std))
    assert all(np.isfinite(s).all() and (s >= 0).all() for s in std)
    assert max(s.max() for s in std) > 0.0
    # moments off: the same chain (the cuts change nothing), so the final paths agree
    a = st["sp"].se.ens.download_paths(L.U, 0)
    b = st2["sp"].se.ens.download_paths(L.U, 0)
    assert np.array_equal(a, b)
