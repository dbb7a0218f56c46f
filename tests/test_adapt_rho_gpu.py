"""ρ access and adaptation on the device (include/dmt.h, "pCN memory ρ") against the oracle, bit
for bit, on the smallest shapes where each draw-kernel family reads ρ:

  c2          W.c2_ou2d(B=150, N=90): register-resident kernels, the service, k_mcmc_resident_pc
  fhnA, fhnB  the ragged FHN pair (7 and 5 multi-segment blocks): wave kernels
  ouA, ouB    the ragged OU pair: scan kernels and k_mcmc_scan
  c5          W.c5_lorenz(B=130, N=70), fp32, MAP_LANE: lane packets

hist_len = 40; no block count is a multiple of 64.  The oracle side (tests/_adapt_oracle.py) runs
without a GPU, so the choice of seeds — that the T3 reference takes every branch of the rule — is
checked by a CPU test here."""
from __future__ import annotations

import numpy as np
import pytest

import diffusionmcmctools_amd as dmt
from diffusionmcmctools_amd import _lib as L
from diffusionmcmctools_amd import workloads as W

import _adapt_oracle as ao
import _cases as cs

CASES = ["c2", "fhnA", "fhnB", "ouA", "ouB", "c5"]
HIST = 40
SEED = 11
# T3 / T4 / T5: every = 8; these ensembles accept most proposals (more at larger ρ), so the band
# sits high: n_lo = 6, n_hi = 7 of 8, both products exact
CFG = ao.config(every=8, lo=0.75, hi=0.875, delta0=0.5, delta_max=0.5, rho_min=0.05, rho_max=0.95)

_LAYOUTS = {
    "A": dict(n_blocks=[2, 3, 2], seg_first=[0, 2, 0, 2, 4, 0, 3], seg_last=[1, 3, 1, 3, 5, 2, 4],
              last=[0, 1, 0, 0, 1, 0, 1], rho=0.7),
    "B": dict(n_blocks=[1, 2, 2], seg_first=[0, 0, 3, 0, 2], seg_last=[3, 2, 5, 1, 4],
              last=[1, 0, 1, 0, 1], rho=0.3),
}
_W = {}


def _workload(case):
    if case not in _W:
        _W[case] = W.c2_ou2d(B=150, N=90) if case == "c2" else W.c5_lorenz(B=130, N=70)
        _W[case].meta["hist_len"] = HIST
    return _W[case]


def _ragged_oracle(model):
    """The oracle half of _cases.ragged_pair (same data, same two layouts), without a device."""
    case = cs.ragged_case(model=model)
    m = case["model"]
    ora = ao.AdaptOracle(m.kind, m.d, m.m, case["n_points"], prec=case["prec"], seed=SEED)
    cs.load_ragged(ora, case)
    ids = []
    for k in ("A", "B"):
        lay = _LAYOUTS[k]
        nb = int(sum(lay["n_blocks"]))
        ids.append((ora.create_layout(lay["n_blocks"], lay["seg_first"], lay["seg_last"],
                                      lay["last"], np.full(nb, lay["rho"]), HIST), nb))
    return ora, ids


def build(case, device=True):
    """(dev or None, oracle, layout, nblocks) with ll computed; device RNG streams of seed 11."""
    if case in ("c2", "c5"):
        w = _workload(case)
        ora = ao.AdaptOracle(w.model.kind, w.d, w.m, w.n_points, prec=w.precision, seed=SEED,
                             grid_shared=w.grid_shared)
        lay, nb, dev = W.fill(ora, w), w.nblocks, None
        if device:
            dev = dmt.Ensemble(w.model.kind, w.d, w.m, w.n_points, precision=w.precision,
                               seed=SEED, grid_shared=w.grid_shared,
                               mapping=L.MAP_LANE if case == "c5" else L.MAP_AUTO)
            assert W.fill(dev, w) == lay
    else:
        model = cs.ou_ragged_model() if case.startswith("ou") else None
        which = 0 if case.endswith("A") else 1
        if device:
            _, dev, ora, ids = cs.ragged_pair(seed=SEED, hist_len=HIST, model=model)
            ao.adopt(ora)
        else:
            dev = None
            ora, ids = _ragged_oracle(model)
        lay, nb = ids[which]
    for e in (dev, ora):
        if e is not None:
            e.loglikhd(lay, L.U, 0, nb)
    return dev, ora, lay, nb


def sub_range(nb):
    return (3, nb - 2) if nb > 7 else (1, nb)


def seeded_rho(n, seed):
    return np.random.default_rng(seed).uniform(0.02, 0.98, n)


def assert_same(dev, ora, lay, nb):
    """ρ, paths, ll, ll° and the three histories, bit for bit."""
    assert np.array_equal(dev.get_rho(lay, 0, nb).view(np.uint64),
                          ora.get_rho(lay, 0, nb).view(np.uint64))
    cs.assert_paths_equal(dev, ora)
    cs.assert_ll_equal(dev, ora, lay, nb)
    for what in (L.BLK_LL_HIST, L.BLK_LLPROP_HIST, L.BLK_ACC_HIST):
        assert np.array_equal(dev.get_block_state(lay, what, 0, nb),
                              ora.get_block_state(lay, what, 0, nb))


def separate_calls(e, lay, nb, i):
    """One iteration as the caller's three calls (on C2: the deferred draw and the service)."""
    e.draw_proposal(lay, 0, nb, iter=i, salt=0)
    e.accept_reject(lay, 0, nb, i, salt=0)
    return e.fetch_ll(lay, 0, nb, i)


# ------------------------------------------------------------------------------------ T3 reference
def t3_reference(case):
    """Oracle side of T3: (oracle, layout, nb, ρ before, counts, ρ after by the Python rule,
    branch names met in the adapted range)."""
    _, ora, lay, nb = build(case, device=False)
    b0, b1 = sub_range(nb)
    rho0 = np.linspace(0.0, 0.999, nb)
    ora.set_rho(lay, 0, nb, rho0)
    ora.mcmc_run(lay, 0, nb, 1, 8)
    counts = ora.accept_counts(lay, 0, nb, 1, 8)
    rho1 = rho0.copy()
    rho1[b0:b1], _ = ao.rule(CFG, 8, rho0[b0:b1], counts[b0:b1])
    met = set()
    for b in range(b0, b1):
        br = ao.branch(CFG, 8, int(counts[b]))
        met.add({1: "up", -1: "down", 0: "unchanged"}[br])
        if br and rho1[b] == CFG["rho_min"]:
            met.add("clamp_min")
        if br and rho1[b] == CFG["rho_max"]:
            met.add("clamp_max")
    return ora, lay, nb, rho0, counts, rho1, met


ALL_BRANCHES = {"up", "down", "unchanged", "clamp_min", "clamp_max"}
# what the oracle alone meets per case (seed 11): the 150- and 130-block cases take every branch;
# the 7- and 5-block layouts cannot (their adapted range starts at block 1, ρ ≥ 0.16)
T3_BRANCHES = {"c2": ALL_BRANCHES, "c5": ALL_BRANCHES}


@pytest.mark.parametrize("case", CASES)
def test_t3_reference_takes_the_branches(case):
    met = t3_reference(case)[6]
    print(case, sorted(met))
    assert met >= T3_BRANCHES.get(case, set()), sorted(met)
    assert {"up", "down"} & met


# ------------------------------------------------------------------------------------ T1
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_t1_set_get_and_draws(case):
    dev, ora, lay, nb = build(case)
    b0, b1 = sub_range(nb)
    before = dev.get_rho(lay, 0, nb)
    assert np.array_equal(before, ora.get_rho(lay, 0, nb))
    rho = seeded_rho(b1 - b0, 1)
    for e in (dev, ora):
        e.set_rho(lay, b0, b1, rho)
    got = dev.get_rho(lay, 0, nb)
    assert np.array_equal(got[b0:b1].view(np.uint64), rho.view(np.uint64))
    assert np.array_equal(got[:b0], before[:b0]) and np.array_equal(got[b1:], before[b1:])
    for i in (1, 2, 3):
        assert dev.mcmc_step(lay, 0, nb, i) == ora.mcmc_step(lay, 0, nb, i)
    assert_same(dev, ora, lay, nb)
    if case == "c2":  # the separate-call loop, ρ replaced between two of its iterations
        for i in (4, 5):
            assert separate_calls(dev, lay, nb, i) == separate_calls(ora, lay, nb, i)
        rho2 = seeded_rho(nb, 2)
        for e in (dev, ora):
            e.set_rho(lay, 0, nb, rho2)
        for i in (6, 7):
            assert separate_calls(dev, lay, nb, i) == separate_calls(ora, lay, nb, i)
        assert_same(dev, ora, lay, nb)
    for bad in ([-0.1], [1.5], [float("nan")]):
        with pytest.raises(dmt.DMTError) as ei:
            dev.set_rho(lay, 0, 1, bad)
        assert ei.value.code == L.ERR_INVALID
    dev.close()


# ------------------------------------------------------------------------------------ T2
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_t2_accept_counts(case):
    dev, _, lay, nb = build(case)
    dev.mcmc_run(lay, 0, nb, 1, 20)
    hist = dev.get_block_state(lay, L.BLK_ACC_HIST, 0, nb)
    assert 0 < hist.sum() < 20 * nb
    b0, b1 = sub_range(nb)
    for i0, i1 in ((1, 1), (5, 12), (1, 20)):
        want = hist[i0 - 1:i1].sum(axis=0, dtype=np.int64)
        got = dev.accept_counts(lay, 0, nb, i0, i1)
        assert got.dtype == np.int64 and np.array_equal(got, want)
        assert np.array_equal(dev.accept_counts(lay, b0, b1, i0, i1), want[b0:b1])
    for i0, i1 in ((0, 4), (5, 4), (1, HIST + 1)):
        with pytest.raises(dmt.DMTError) as ei:
            dev.accept_counts(lay, 0, nb, i0, i1)
        assert ei.value.code == L.ERR_INVALID
    with pytest.raises(dmt.DMTError) as ei:  # layout 0 (whole recordings) keeps no histories
        dev.accept_counts(0, 0, 1, 1, 1)
    assert ei.value.code == L.ERR_STATE
    dev.close()


# ------------------------------------------------------------------------------------ T3
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_t3_adapt_rho(case):
    ora, lay, nb, rho0, counts, rho1, met = t3_reference(case)
    assert met >= T3_BRANCHES.get(case, set())
    dev = build(case)[0]
    b0, b1 = sub_range(nb)
    dev.set_rho(lay, 0, nb, rho0)
    dev.mcmc_run(lay, 0, nb, 1, 8)
    got_counts = dev.accept_counts(lay, 0, nb, 1, 8)
    assert np.array_equal(got_counts, counts)
    n = dev.adapt_rho(lay, b0, b1, 8, CFG)
    got = dev.get_rho(lay, 0, nb)
    # the device's ρ = the host rule (libdmt's and the Python restatement) on the counts
    want, _ = dmt.adapt_rule(CFG, 8, rho0[b0:b1], got_counts[b0:b1])
    assert np.array_equal(got[b0:b1].view(np.uint64), want.view(np.uint64))
    assert np.array_equal(got.view(np.uint64), rho1.view(np.uint64))
    assert np.array_equal(got[:b0], rho0[:b0]) and np.array_equal(got[b1:], rho0[b1:])
    assert n == int((rho1 != rho0).sum()) == ora.adapt_rho(lay, b0, b1, 8, CFG)
    # sqrt(1 − ρ²) as the device formed it: one more draw equals the oracle's
    assert dev.mcmc_step(lay, 0, nb, 9) == ora.mcmc_step(lay, 0, nb, 9)
    assert_same(dev, ora, lay, nb)
    # not on the grid of `every`, window before iteration 1, no histories
    for it, cfg in ((7, CFG), (0, CFG), (8, dict(CFG, every=16)), (8, dict(CFG, delta0=0.0))):
        with pytest.raises(dmt.DMTError) as ei:
            dev.adapt_rho(lay, 0, nb, it, cfg)
        assert ei.value.code == L.ERR_INVALID
    with pytest.raises(dmt.DMTError) as ei:
        dev.adapt_rho(0, 0, 1, 8, CFG)
    assert ei.value.code == L.ERR_STATE
    assert dev.adapt_rho(lay, 0, nb, 16, dict(CFG, until=8)) == 0  # ended: nothing moves
    assert np.array_equal(dev.get_rho(lay, 0, nb), got)
    dev.close()


# ------------------------------------------------------------------------------------ T4, T5
_RUN = {}


def run_reference(case, until=0):
    """The oracle's mcmc_run(3, 30) with adaptation every 8 installed, once per case:
    per-iteration results, final ρ, and the oracle itself (left unchanged afterwards)."""
    key = (case, until)
    if key not in _RUN:
        _, ora, lay, nb = build(case, device=False)
        ora.set_run_adaptation(lay, dict(CFG, until=until))
        out = ora.mcmc_run(lay, 0, nb, 3, 30)
        _RUN[key] = (ora, lay, nb, out)
    return _RUN[key]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_t4_adaptation_inside_the_run(case):
    ora, lay, nb, want = run_reference(case)
    a = build(case)[0]
    b = build(case)[0]
    rho_init = a.get_rho(lay, 0, nb)
    a.set_run_adaptation(lay, CFG)
    ra = a.mcmc_run(lay, 0, nb, 3, 30)
    rb = []
    for i0, i1 in ((3, 8), (9, 16), (17, 24), (25, 32)):
        rb.append(b.mcmc_run(lay, 0, nb, i0, i1 - i0 + 1))
        b.adapt_rho(lay, 0, nb, i1, CFG, want_changed=False)
    rb = np.concatenate(rb)
    assert np.array_equal(ra, rb) and np.array_equal(ra, want)
    assert not np.array_equal(a.get_rho(lay, 0, nb), rho_init)  # ρ did move
    assert_same(a, ora, lay, nb)
    assert_same(b, ora, lay, nb)
    # off again: the next run is one piece and ρ stays
    a.set_run_adaptation(lay, None)
    rho = a.get_rho(lay, 0, nb)
    a.mcmc_run(lay, 0, nb, 33, 8)
    assert np.array_equal(a.get_rho(lay, 0, nb), rho)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["c2", "fhnA", "c5"])
def test_t4_with_run_snapshots(case):
    """Snapshots every 5 and adaptation every 8 in one run: one cut loop serves both."""
    ora, lay, nb, want = run_reference(case)
    a = build(case)[0]
    b = build(case)[0]
    a.snapshot_reserve(6, what_mask=3)
    a.set_run_snapshots(5, slot0=0)
    a.set_run_adaptation(lay, CFG)
    ra = a.mcmc_run(lay, 0, nb, 3, 30)
    assert np.array_equal(ra, want)
    assert_same(a, ora, lay, nb)
    cuts = sorted(set(range(5, 33, 5)) | set(range(8, 33, 8)))
    ref, i0 = {}, 3
    for i1 in cuts:
        b.mcmc_run(lay, 0, nb, i0, i1 - i0 + 1)
        if i1 % 5 == 0:  # the stopped run's u, before the adaptation of the same iteration
            ref[i1] = (b.download_paths(L.U, 0), b.download_paths(L.U, 1))
        if i1 % 8 == 0:
            b.adapt_rho(lay, 0, nb, i1, CFG)
        i0 = i1 + 1
    for slot, it in enumerate(range(5, 31, 5)):
        X, got_it = a.snapshot_download(slot, 0)
        Wc, _ = a.snapshot_download(slot, 1)
        assert got_it == it
        assert np.array_equal(X, ref[it][0]) and np.array_equal(Wc, ref[it][1])
    a.set_run_snapshots(0)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["c2", "ouB", "c5"])
def test_t4_until(case):
    ora, lay, nb, want = run_reference(case, until=16)
    a = build(case)[0]
    a.set_run_adaptation(lay, dict(CFG, until=16))
    r1 = a.mcmc_run(lay, 0, nb, 3, 14)
    rho16 = a.get_rho(lay, 0, nb)
    r2 = a.mcmc_run(lay, 0, nb, 17, 16)
    assert np.array_equal(np.concatenate([r1, r2]), want)
    assert np.array_equal(a.get_rho(lay, 0, nb).view(np.uint64), rho16.view(np.uint64))
    assert not np.array_equal(rho16, build(case, device=False)[1].get_rho(lay, 0, nb))
    assert_same(a, ora, lay, nb)
    a.close()


@pytest.mark.gpu
def test_t5_service_loop():
    """The caller's separate calls (C2: deferred draws, the resident service) with adapt_rho
    after iterations 8, 16, 24 and 32 equal the adapted run of T4: the service restarts with the
    new ρ."""
    ora, lay, nb, want = run_reference("c2")
    dev = build("c2")[0]
    out = []
    for i in range(3, 33):
        out.append(separate_calls(dev, lay, nb, i))
        if i % 8 == 0:
            dev.adapt_rho(lay, 0, nb, i, CFG, want_changed=False)
    assert np.array_equal(np.array(out, dtype=np.float64), want)
    assert_same(dev, ora, lay, nb)
    st = dev.service_stats()
    print("service:", st)
    dev.close()
