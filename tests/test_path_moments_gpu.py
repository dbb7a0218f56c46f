"""Posterior path moments on the device (include/dmt.h, "posterior path moments"): the running
mean and sum of squared deviations of u.XX against the NumPy fold of tests/_moments_ref.py, bit
for bit, on the smallest shapes where each geometry of the planes can go wrong (no recording
count is a multiple of 64, no length a multiple of 32):

  c2          W.c2_ou2d(B=150, N=90)                tw = 1, single segment, resident kernels
  ouA_ouB     ragged OU pair, two blockings         tw = 1, multi-segment, scan kernels
  fhn_wave    ragged FHN pair, default mapping      tw = 1, FHN
  fhn_lane    ragged FHN pair, MAP_LANE             tw = 64, three path buffers, ragged
  c3_lane     W.c3_fhn(B=130, N=150), MAP_LANE      tw = 64, two full tiles + 2
  f32_ragged  ragged FHN pair, fp32, MAP_LANE       packets, segments straddling packets
  c5          W.c5_lorenz(B=130, N=70), MAP_LANE    packets, partial last packet and tile

The seeds (that accepted and rejected blocks, and differing selectors, occur) are checked on the
oracle twins by tests/test_path_moments.py and again here on the device's own accpt_history."""
from __future__ import annotations

import numpy as np
import pytest

import diffusionmcmctools_amd as dmt
from diffusionmcmctools_amd import _lib as L
from diffusionmcmctools_amd import engine as E

import _adapt_oracle as ao
import _moments_ref as mr

pytestmark = pytest.mark.gpu


def _dev(case):
    dev, _, plan = mr.build(case, oracle=False)
    return dev, plan


def _state(e, plan):
    """Everything an accumulation must leave alone."""
    out = [e.download_paths(u, what) for u in (L.U, L.UPROP) for what in (0, 1, 2)]
    for lay, nb in plan:
        out += [e.get_block_state(lay, what, 0, nb)
                for what in (L.BLK_LL, L.BLK_LLPROP, L.BLK_LL_HIST, L.BLK_LLPROP_HIST,
                             L.BLK_ACC_HIST)]
    return out, e.rng_state()


def _assert_state_equal(a, b):
    assert a[1] == b[1]
    assert len(a[0]) == len(b[0])
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y, equal_nan=True)


def _assert_moments(e, mean, m2, n, last=None):
    dm, ds, dn = e.moments_download()
    assert dn == n
    if last is not None:
        assert e.moments_state() == (n, last)
    assert np.array_equal(mr.bits(dm), mr.bits(mean)), \
        f"mean differs at {np.argwhere(mr.bits(dm) != mr.bits(mean))[:4].tolist()}"
    assert np.array_equal(mr.bits(ds), mr.bits(m2)), \
        f"m2 differs at {np.argwhere(mr.bits(ds) != mr.bits(m2))[:4].tolist()}"


# ------------------------------------------------------------------ 1. accumulate equals the fold
@pytest.mark.parametrize("case", mr.CASES)
def test_accumulate_equals_the_fold(case):
    dev, plan = _dev(case)
    dev.moments_reserve()
    xs = []
    for i in range(1, 11):
        mr.step(dev, plan, i, case in mr.RAGGED)
        dev.moments_accumulate(i)
        xs.append(dev.download_paths(L.U, 0))
    mean, m2, n = mr.fold(xs)
    assert n == 10
    _assert_moments(dev, mean, m2, 10, last=10)
    mr.check_seed_condition(dev, case, plan, list(range(1, 11)))
    dev.close()


def test_accumulate_after_separate_calls_deferred_draw_and_service():
    """C2 as the caller's three calls per iteration (the deferred draw, fused with its accept, on
    the resident service): an accumulation stops the service first; one that falls between a draw
    and its accept launches the deferred draw first, which leaves u alone."""
    dev, plan = _dev("c2")
    lay, nb = plan[0]
    dev.moments_reserve()
    xs = []
    for i in range(1, 13):
        dev.draw_proposal(lay, 0, nb, iter=i, salt=0)
        if i == 7:  # between the draw and its accept: u is still iteration 6's
            dev.moments_accumulate(100 + i)
            xs.append(xs[-1])
        dev.accept_reject(lay, 0, nb, i, salt=0)
        dev.fetch_ll(lay, 0, nb, i)
        if i % 3 == 0:  # after three consecutive fused iterations: the service is running
            dev.moments_accumulate(i)
            xs.append(dev.download_paths(L.U, 0))
    st = dev.service_stats()
    print("service stats:", st)
    assert st["starts"] >= 1 and st["posts"] >= 2, st
    mean, m2, n = mr.fold(xs)
    _assert_moments(dev, mean, m2, n, last=12)
    assert n == 5
    dev.close()


# ------------------------------------------------------------------ 2. inside mcmc_run
def _single_plan(case, e, plan):
    lay, nb = plan[0]
    if case in mr.RAGGED:
        e.loglikhd(lay, L.U, 0, nb)
    return lay, nb


def _assert_twins_equal(e0, e1, lay, nb):
    a, b = _state(e0, [(lay, nb)]), _state(e1, [(lay, nb)])
    _assert_state_equal(a, b)


@pytest.mark.parametrize("case", ["c2", "fhn_lane", "c5"])
def test_moments_inside_mcmc_run(case):
    e0, plan = _dev(case)
    e1, _ = _dev(case)
    lay, nb = _single_plan(case, e0, plan)
    _single_plan(case, e1, plan)
    e0.moments_reserve()
    e0.set_run_moments(3, 6)
    out0 = e0.mcmc_run(lay, 0, nb, 3, 23)
    outs, xs, it = [], [], 3
    for end in (6, 9, 12, 15, 18, 21, 24, 25):
        outs.append(e1.mcmc_run(lay, 0, nb, it, end - it + 1))
        it = end + 1
        if end % 3 == 0:
            xs.append(e1.download_paths(L.U, 0))
    assert len(xs) == 7
    assert np.array_equal(out0, np.concatenate(outs))
    mean, m2, n = mr.fold(xs)
    _assert_moments(e0, mean, m2, 7, last=24)
    _assert_twins_equal(e0, e1, lay, nb)
    e0.close()
    e1.close()


def test_moments_with_snapshots_and_adaptation_inside_mcmc_run():
    """C2 with run snapshots (every 5), moments (every 3 from 6) and adaptation of ρ (every 8)
    installed together: the run equals the loop of shorter runs and explicit calls in the
    documented order — snapshot, moments, adaptation."""
    cfg = ao.config(every=8, lo=0.75, hi=0.875)
    e0, plan = _dev("c2")
    e1, _ = _dev("c2")
    lay, nb = plan[0]
    for e in (e0, e1):
        e.snapshot_reserve(8)
        e.moments_reserve()
    e0.set_run_snapshots(5, 0)
    e0.set_run_adaptation(lay, cfg)
    e0.set_run_moments(3, 6)
    out0 = e0.mcmc_run(lay, 0, nb, 3, 23)
    outs, it, slot = [], 3, 0
    cuts = sorted({i for i in range(3, 26) if i % 5 == 0 or i % 8 == 0 or (i % 3 == 0 and i >= 6)}
                  | {25})
    for end in cuts:
        outs.append(e1.mcmc_run(lay, 0, nb, it, end - it + 1))
        it = end + 1
        if end % 5 == 0:
            e1.snapshot_take(slot, end)
            slot += 1
        if end % 3 == 0 and end >= 6:
            e1.moments_accumulate(end)
        if end % 8 == 0:
            e1.adapt_rho(lay, 0, nb, end, cfg, want_changed=False)
    assert np.array_equal(out0, np.concatenate(outs))
    m1, s1, n1 = e1.moments_download()
    assert n1 == 7
    _assert_moments(e0, m1, s1, 7, last=24)
    assert slot == 5
    for s in range(slot):
        a, ia = e0.snapshot_download(s)
        b, ib = e1.snapshot_download(s)
        assert ia == ib == 5 * (s + 1) and np.array_equal(a, b)
    assert np.array_equal(e0.get_rho(lay, 0, nb).view(np.uint64),
                          e1.get_rho(lay, 0, nb).view(np.uint64))
    assert not np.array_equal(e0.get_rho(lay, 0, nb), np.full(nb, e0.get_rho(lay, 0, 1)[0]))
    _assert_twins_equal(e0, e1, lay, nb)
    e0.close()
    e1.close()


# ------------------------------------------------------------------ 3. nothing else moves
@pytest.mark.parametrize("case", ["c2", "f32_ragged"])
def test_accumulate_leaves_everything_else_alone(case):
    dev, plan = _dev(case)
    for i in range(1, 5):
        lay, nb = plan[(i - 1) % len(plan)]
        if case in mr.RAGGED:
            dev.loglikhd(lay, L.U, 0, nb)
        dev.mcmc_run(lay, 0, nb, i, 1, salt=L.RNG_AUTO)
    dev.moments_reserve()
    before = _state(dev, plan)
    dev.moments_accumulate(4)
    after = _state(dev, plan)
    _assert_state_equal(before, after)
    assert dev.moments_state() == (1, 4)
    dev.close()


@pytest.mark.parametrize("case", ["c2", "f32_ragged"])
def test_run_with_moments_equals_run_without(case):
    e0, plan = _dev(case)
    e1, _ = _dev(case)
    lay, nb = _single_plan(case, e0, plan)
    _single_plan(case, e1, plan)
    e0.moments_reserve()
    e0.set_run_moments(2, 0)
    out0 = e0.mcmc_run(lay, 0, nb, 1, 9, salt=L.RNG_AUTO)
    out1 = e1.mcmc_run(lay, 0, nb, 1, 9, salt=L.RNG_AUTO)
    assert np.array_equal(out0, out1)
    assert e0.moments_state() == (4, 8)
    _assert_twins_equal(e0, e1, lay, nb)
    e0.close()
    e1.close()


# ------------------------------------------------------------------ 4. checkpoint
@pytest.mark.parametrize("case", ["fhn_lane", "c5"])
def test_checkpoint_resumes_bit_for_bit(case):
    e0, plan = _dev(case)
    e1, _ = _dev(case)
    ragged = case in mr.RAGGED
    e0.moments_reserve()
    e1.moments_reserve()
    for i in range(1, 11):  # e1: ten accumulations, uninterrupted
        mr.step(e1, plan, i, ragged)
        e1.moments_accumulate(i)
    for i in range(1, 6):
        mr.step(e0, plan, i, ragged)
        e0.moments_accumulate(i)
    mean, m2, n = e0.moments_download()
    assert n == 5
    e0.moments_reserve()  # zeroes
    z, zs, zn = e0.moments_download()
    assert zn == 0 and not z.any() and not zs.any() and e0.moments_state() == (0, 0)
    e0.moments_upload(mean, m2, n)
    for i in range(6, 11):
        mr.step(e0, plan, i, ragged)
        e0.moments_accumulate(i)
    m1, s1, n1 = e1.moments_download()
    assert n1 == 10
    _assert_moments(e0, m1, s1, 10, last=10)
    # arbitrary arrays survive upload + download, and one more accumulation is the host rule
    rng = np.random.default_rng(5)
    rm = rng.standard_normal(mean.shape) * 3.0
    rs = rng.uniform(0.0, 50.0, mean.shape)
    e0.moments_upload(rm, rs, 41)
    _assert_moments(e0, rm, rs, 41)
    e0.moments_accumulate(11)
    x = e0.download_paths(L.U, 0)
    hm, hs = E.moments_rule(x, rm, rs, 42)
    _assert_moments(e0, hm.reshape(mean.shape), hs.reshape(mean.shape), 42, last=11)
    e0.close()
    e1.close()


# ------------------------------------------------------------------ 5. errors and accounting
def _code(fn, *a, **k):
    with pytest.raises(dmt.DMTError) as ei:
        fn(*a, **k)
    return ei.value.code


def test_errors():
    dev, plan = _dev("c2")
    z = np.zeros((dev.P, dev.d))
    assert _code(dev.moments_accumulate, 1) == L.ERR_STATE
    assert _code(dev.moments_reset) == L.ERR_STATE
    assert _code(dev.moments_state) == L.ERR_STATE
    assert _code(dev.moments_download) == L.ERR_STATE
    assert _code(dev.moments_upload, z, z, 0) == L.ERR_STATE
    assert _code(dev.set_run_moments, 3, 0) == L.ERR_STATE
    dev.set_run_moments(0, 0)  # off needs no reserve
    assert _code(dev.set_run_moments, -1, 0) == L.ERR_INVALID
    assert _code(dev.set_run_moments, 3, -1) == L.ERR_INVALID
    dev.moments_reserve()
    assert _code(dev.moments_upload, z, z, -1) == L.ERR_INVALID
    assert _code(dev.set_run_moments, -2, 0) == L.ERR_INVALID
    dev.set_run_moments(3, 0)
    dev.moments_reserve(False)
    assert _code(dev.moments_accumulate, 1) == L.ERR_STATE
    lay, nb = plan[0]
    dev.mcmc_run(lay, 0, nb, 1, 3)  # freeing turned the run moments off
    dev.close()


@pytest.mark.parametrize("case", ["c2", "c5"])
def test_memory_accounting(case):
    dev, plan = _dev(case)
    b0 = dev.memory_bytes()
    dev.moments_reserve()
    b1 = dev.memory_bytes()
    if case == "c2":  # tw = 1: a tile per recording of Q + 32 spare rows, d components, 8 bytes
        assert b1 - b0 == 2 * 150 * (91 + 32) * 2 * 8
    assert b1 - b0 >= 2 * dev.P * dev.d * 8 and (b1 - b0) % 16 == 0
    dev.moments_reserve()  # zeroes, no second allocation
    assert dev.memory_bytes() == b1
    dev.moments_accumulate(1)
    dev.moments_reset()
    assert dev.moments_state() == (0, 0) and dev.memory_bytes() == b1
    dev.moments_reserve(False)
    assert dev.memory_bytes() == b0
    dev.close()


def test_timing_counts_one_launch_per_accumulate():
    dev, plan = _dev("fhn_lane")
    dev.moments_reserve()
    dev.set_timing(True)
    for i in range(1, 4):
        dev.moments_accumulate(i)
    ms, count = dev.get_timing(L.K_MOMENTS)
    assert count == 3 and ms > 0.0
    assert dev.get_timing(L.K_DRAW)[1] == 0
    assert "k_path_moments" in L.recent_kernels()[0]
    dev.close()


# ------------------------------------------------------------------ 6. high-level API
def test_api_on_device_and_oracle_engine():
    dev, ora, plan = mr.build("fhn_wave")
    data = mr.cs.ragged_case()
    ses = [dmt.SamplingEnsemble(data["model"], data["n_points"], _engine=e) for e in (dev, ora)]
    got = []
    for se in ses:
        se.reserve_path_moments()
        for i in range(1, 7):
            mr.step(se.ens, plan, i, True)
            se.accumulate_path_moments(i)
        got.append(se.path_moments())
    (md, vd, nd), (mo, vo, no) = got
    assert nd == no == 6
    for a, b in ((md, mo), (vd, vo)):
        assert [len(r) for r in a] == [len(r) for r in b] == [4, 6, 5]
        for ra, rb in zip(a, b):
            for sa, sb in zip(ra, rb):
                assert sa.shape == sb.shape and np.array_equal(mr.bits(sa), mr.bits(sb))
    mean, m2, n = dev.moments_download()
    assert np.array_equal(mr.bits(np.concatenate([s for r in vd for s in r])), mr.bits(m2 / 5))
    assert np.array_equal(mr.bits(np.concatenate([s for r in md for s in r])), mr.bits(mean))
    dev.close()
