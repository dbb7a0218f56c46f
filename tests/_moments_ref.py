"""The reference side of the path-moment tests: the rule of include/dmt.h ("posterior path
moments") restated in NumPy, the cases of the GPU tests and the drivers both the device and its
oracle twin run, so that the choice of seeds can be checked without a GPU.  Test infrastructure."""
from __future__ import annotations

import numpy as np

from diffusionmcmctools_amd import _lib as L
from diffusionmcmctools_amd import workloads as W

import _cases as cs

SEED = 11
HIST = 32  # history rows of every layout (the longest test runs iterations 1..25)


# ------------------------------------------------------------------------------------ the rule
def rule(x, mean, m2, n):
    """Welford's update of float64 arrays, every operation its own ufunc call (one rounding
    each); n is the new count (a Python int, converted to float64)."""
    x = np.asarray(x, dtype=np.float64)
    mean = np.asarray(mean, dtype=np.float64)
    m2 = np.asarray(m2, dtype=np.float64)
    nn = np.float64(int(n))
    delta = np.subtract(x, mean)
    mean1 = np.add(mean, np.divide(delta, nn))
    m21 = np.add(m2, np.multiply(delta, np.subtract(x, mean1)))
    return mean1, m21


def fold(samples, mean=None, m2=None, n=0):
    """(mean, m2, n) after folding the samples in order, from zeros or from (mean, m2, n)."""
    samples = [np.asarray(s, dtype=np.float64) for s in samples]
    mean = np.zeros_like(samples[0]) if mean is None else np.array(mean, dtype=np.float64)
    m2 = np.zeros_like(samples[0]) if m2 is None else np.array(m2, dtype=np.float64)
    for s in samples:
        n += 1
        mean, m2 = rule(s, mean, m2, n)
    return mean, m2, n


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------ the cases
# name -> geometry of the device planes it exercises (include/dmt.h, DESIGN.md "path moments")
CASES = ["c2", "ouA_ouB", "fhn_wave", "fhn_lane", "c3_lane", "f32_ragged", "c5"]
RAGGED = {"ouA_ouB", "fhn_wave", "fhn_lane", "f32_ragged"}
_W = {}


def _workload(case):
    if case not in _W:
        _W[case] = {"c2": lambda: W.c2_ou2d(B=150, N=90),
                    "c3_lane": lambda: W.c3_fhn(B=130, N=150, T_burn=0.1),
                    "c5": lambda: W.c5_lorenz(B=130, N=70)}[case]()
        _W[case].meta["hist_len"] = HIST
    return _W[case]


def _ragged_kw(case):
    return {"ouA_ouB": dict(model=cs.ou_ragged_model()),
            "fhn_wave": dict(),
            "fhn_lane": dict(mapping=L.MAP_LANE),
            "f32_ragged": dict(prec=L.F32, mapping=L.MAP_LANE)}[case]


def _ragged_oracle(case):
    """The oracle half of _cases.ragged_pair (same data, same two layouts), without a device."""
    import oracle as orc
    kw = _ragged_kw(case)
    data = cs.ragged_case(model=kw.get("model"), prec=kw.get("prec", L.F64))
    m = data["model"]
    ora = orc.OracleEnsemble(m.kind, m.d, m.m, data["n_points"], prec=data["prec"], seed=SEED)
    cs.load_ragged(ora, data)
    layA = dict(n_blocks=[2, 3, 2], seg_first=[0, 2, 0, 2, 4, 0, 3], seg_last=[1, 3, 1, 3, 5, 2, 4],
                last=[0, 1, 0, 0, 1, 0, 1])
    layB = dict(n_blocks=[1, 2, 2], seg_first=[0, 0, 3, 0, 2], seg_last=[3, 2, 5, 1, 4],
                last=[1, 0, 1, 0, 1])
    ids = []
    for lay, rho in ((layA, 0.7), (layB, 0.3)):
        nb = int(sum(lay["n_blocks"]))
        ids.append((ora.create_layout(lay["n_blocks"], lay["seg_first"], lay["seg_last"],
                                      lay["last"], np.full(nb, rho), HIST), nb))
    return ora, ids


def build(case, device=True, oracle=True):
    """(dev or None, oracle or None, plan): plan = [(layout, nblocks), ...], the layouts the
    iterations alternate (one for the single-layout cases).  Device RNG streams of SEED."""
    import oracle as orc
    if case in RAGGED:
        if device:
            _, dev, ora, plan = cs.ragged_pair(seed=SEED, hist_len=HIST, **_ragged_kw(case))
        else:
            dev = None
            ora, plan = _ragged_oracle(case)
        return dev, (ora if oracle else None), plan
    import diffusionmcmctools_amd as dmt
    w = _workload(case)
    dev = ora = None
    lay = None
    if oracle:
        ora = orc.OracleEnsemble(w.model.kind, w.d, w.m, w.n_points, prec=w.precision, seed=SEED,
                                 grid_shared=w.grid_shared)
        lay = W.fill(ora, w)
    if device:
        dev = dmt.Ensemble(w.model.kind, w.d, w.m, w.n_points, precision=w.precision, seed=SEED,
                           grid_shared=w.grid_shared,
                           mapping=L.MAP_AUTO if case == "c2" else L.MAP_LANE)
        lay_d = W.fill(dev, w)
        assert lay is None or lay == lay_d
        lay = lay_d
    for e in (dev, ora):
        if e is not None:
            e.loglikhd(lay, L.U, 0, w.nblocks)
    return dev, ora, [(lay, w.nblocks)]


def segments_of_blocks(e, case):
    """Per layout of the plan: for every block, the global ids of its segments."""
    if case not in RAGGED:
        return [[[b] for b in range(_workload(case).nblocks)]]
    nseg = [4, 6, 5]
    first = np.concatenate([[0], np.cumsum(nseg)])
    out = []
    for lay in (dict(n_blocks=[2, 3, 2], seg_first=[0, 2, 0, 2, 4, 0, 3], seg_last=[1, 3, 1, 3, 5, 2, 4]),
                dict(n_blocks=[1, 2, 2], seg_first=[0, 0, 3, 0, 2], seg_last=[3, 2, 5, 1, 4])):
        blocks, b = [], 0
        for r, nb in enumerate(lay["n_blocks"]):
            for _ in range(nb):
                blocks.append(list(range(first[r] + lay["seg_first"][b],
                                         first[r] + lay["seg_last"][b] + 1)))
                b += 1
        out.append(blocks)
    return out


def step(e, plan, i, ragged):
    """Iteration i as a one-iteration mcmc_run on the layout whose turn it is (the ragged pairs
    alternate their two blockings, recomputing the blocks' ll first, as
    biblock/smoothing_with_blocking.md does)."""
    lay, nb = plan[(i - 1) % len(plan)]
    if ragged:
        e.loglikhd(lay, L.U, 0, nb)
    return e.mcmc_run(lay, 0, nb, i, 1)


def accepted_rows(e, plan, iters):
    """accpt_history row of each iteration in `iters`, from the layout that ran it."""
    hist = [e.get_block_state(lay, L.BLK_ACC_HIST, 0, nb) for lay, nb in plan]
    return [np.asarray(hist[(i - 1) % len(plan)][i - 1]).astype(bool) for i in iters]


def check_seed_condition(e, case, plan, iters):
    """The iterations in `iters` hold an accepted and a rejected block-iteration, and — ragged
    cases — at some of them the segments' path selectors differ: a segment's u changes buffer
    exactly when its block accepts, so the selectors differ once the per-segment accept counts
    up to that iteration have different parities.  A kernel that ignored the selectors, or read
    every point from one buffer, cannot pass a case that meets this."""
    rows = accepted_rows(e, plan, iters)
    flat = np.concatenate(rows)
    assert flat.any(), f"{case}: no block-iteration accepted"
    assert (~flat).any(), f"{case}: no block-iteration rejected"
    if case not in RAGGED:
        return
    segs = segments_of_blocks(e, case)
    G = 1 + max(g for blocks in segs for b in blocks for g in b)
    parity = np.zeros(G, dtype=np.int64)
    differ = False
    for i, row in zip(iters, rows):  # iters: every iteration run so far, in order, all accumulated
        for b, acc in enumerate(row):
            if acc:
                parity[segs[(i - 1) % len(plan)][b]] ^= 1
        differ = differ or len(set(parity.tolist())) > 1
    assert differ, f"{case}: every segment's selector agrees at every accumulated iteration"
