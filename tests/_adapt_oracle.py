"""The oracle side of the pCN-memory tests: the adaptation rule of include/dmt.h ("pCN memory
ρ") restated in pure Python (libm's exp and sqrt through ``math``, IEEE double arithmetic), and
an OracleEnsemble that reads, writes and adapts its blocks' ρ with it — the same call surface as
``engine.Ensemble``.  Test infrastructure."""
from __future__ import annotations

import math

import numpy as np

import oracle as orc

def config(every, lo=0.25, hi=0.5, delta0=0.5, delta_max=0.5, rho_min=0.05, rho_max=0.95, until=0):
    return dict(every=int(every), lo=float(lo), hi=float(hi), delta0=float(delta0),
                delta_max=float(delta_max), rho_min=float(rho_min), rho_max=float(rho_max),
                until=int(until))


def check_config(c):
    ok = (c["every"] >= 1 and 0.0 <= c["lo"] <= c["hi"] <= 1.0
          and math.isfinite(c["delta0"]) and c["delta0"] > 0.0
          and math.isfinite(c["delta_max"]) and c["delta_max"] > 0.0
          and 0.0 <= c["rho_min"] <= c["rho_max"] <= 1.0 and c["until"] >= 0)
    if not ok:
        raise ValueError("invalid adaptation config")


def step(c, mcmciter):
    """(κ_up, κ_dn, n_lo, n_hi) of the adaptation after iteration mcmciter."""
    check_config(c)
    if mcmciter < 1 or mcmciter % c["every"] != 0:
        raise ValueError("mcmciter must be a positive multiple of every")
    k = mcmciter // c["every"]
    delta = min(c["delta_max"], c["delta0"] / math.sqrt(float(k)))
    return (math.exp(delta), math.exp(-delta), int(math.ceil(c["lo"] * c["every"])),
            int(math.floor(c["hi"] * c["every"])))


def branch(c, mcmciter, count):
    """+1 (κ_up), −1 (κ_dn) or 0 (in the band, or adaptation has ended)."""
    _, _, n_lo, n_hi = step(c, mcmciter)
    if c["until"] > 0 and mcmciter > c["until"]:
        return 0
    return 1 if count < n_lo else (-1 if count > n_hi else 0)


def rule_one(c, mcmciter, rho, count):
    """ρ', sqrt(1 − ρ'²), or None for a block the rule leaves alone."""
    k_up, k_dn, n_lo, n_hi = step(c, mcmciter)
    if c["until"] > 0 and mcmciter > c["until"]:
        return None
    if count < n_lo:
        kap = k_up
    elif count > n_hi:
        kap = k_dn
    else:
        return None
    num = kap * rho
    den = num + (1.0 - rho)
    rn = num / den if den != 0.0 else math.nan
    rn = rn if rn > c["rho_min"] else c["rho_min"]
    rn = rn if rn < c["rho_max"] else c["rho_max"]
    return rn, math.sqrt(1.0 - rn * rn)


def rule(c, mcmciter, rho, counts):
    """dmt_adapt_rule restated: (ρ', sqrt(1 − ρ'²)) arrays."""
    out, sout = [], []
    for r, n in zip(np.asarray(rho, dtype=np.float64).tolist(), np.asarray(counts).tolist()):
        if not 0.0 <= r <= 1.0:
            raise ValueError("rho outside [0,1]")
        got = rule_one(c, mcmciter, r, int(n))
        if got is None:
            got = (r, math.sqrt(1.0 - r * r))
        out.append(got[0])
        sout.append(got[1])
    return np.array(out), np.array(sout)


class AdaptOracle(orc.OracleEnsemble):
    """OracleEnsemble + ρ access and adaptation (its blocks' rho / srho are plain attributes)."""

    def __init__(self, *a, **k):
        self._adapt = {}
        super().__init__(*a, **k)

    def get_rho(self, layout, b0, b1):
        return np.array([b.rho for b in self.layouts[layout][b0:b1]])

    def set_rho(self, layout, b0, b1, rho):
        v = np.broadcast_to(np.asarray(rho, dtype=np.float64), (b1 - b0,))
        if not np.all((v >= 0.0) & (v <= 1.0)):
            raise ValueError("rho outside [0,1]")
        for b, r in zip(self.layouts[layout][b0:b1], v.tolist()):
            b.rho = r
            b.srho = math.sqrt(1.0 - r * r)

    def accept_counts(self, layout, b0, b1, i0, i1):
        bks = self.layouts[layout]
        if not 1 <= i0 <= i1 <= (len(bks[0].acc_hist) if bks else 0):
            raise ValueError("iterations outside 1:ll_hist_len")
        return np.array([int(np.count_nonzero(b.acc_hist[i0 - 1:i1]))
                         for b in self.layouts[layout][b0:b1]], dtype=np.int64)

    def adapt_rho(self, layout, b0, b1, mcmciter, cfg, want_changed=True):
        step(cfg, mcmciter)  # validates
        counts = self.accept_counts(layout, b0, b1, mcmciter - cfg["every"] + 1, mcmciter)
        changed = 0
        for b, n in zip(self.layouts[layout][b0:b1], counts.tolist()):
            got = rule_one(cfg, mcmciter, b.rho, n)
            if got is not None:
                changed += got[0] != b.rho
                b.rho, b.srho = got
        return int(changed) if want_changed else None

    def set_run_adaptation(self, layout, cfg):
        if cfg is None or cfg["every"] == 0:
            self._adapt.pop(layout, None)
            return
        check_config(cfg)
        self._adapt[layout] = dict(cfg)

    def mcmc_run(self, layout, b0, b1, iter0, n_iter, salt=0, local=False):
        cfg = self._adapt.get(layout)
        if cfg is None:
            return super().mcmc_run(layout, b0, b1, iter0, n_iter, salt=salt, local=local)
        out, done, ev = [], 0, cfg["every"]
        while done < n_iter:
            it = iter0 + done
            cut = -(-it // ev) * ev
            due = cfg["until"] == 0 or cut <= cfg["until"]
            n = min(n_iter - done, cut - it + 1) if due else n_iter - done
            out.append(super().mcmc_run(layout, b0, b1, it, n, salt=salt, local=local))
            done += n
            last = iter0 + done - 1
            if due and last == cut:
                self.adapt_rho(layout, b0, b1, last, cfg)
        return np.concatenate(out)


def adopt(ora):
    """Turn an OracleEnsemble built elsewhere (e.g. by _cases.ragged_pair) into an AdaptOracle."""
    ora.__class__ = AdaptOracle
    ora._adapt = {}
    return ora
