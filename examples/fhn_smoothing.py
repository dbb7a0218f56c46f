"""The smoothing tutorial (docs/src/tutorials/biblock/smoothing.md:25-58) on the preamble's FHN
data, returning the smoothing estimate itself instead of a cloud of kept paths.

The tutorial keeps ``deepcopy(bb.b.XX)`` every 400 iterations and plots the cloud.  Here the
posterior mean path and its pointwise standard deviation come from the path moments the engine
accumulates on the device (``SamplingEnsemble.path_moments_every``): after a burn-in, every
``every``-th accepted path is folded into a running mean and a running sum of squared deviations
inside ``mcmc_run``, with no download of ``XX``.

    python examples/fhn_smoothing.py [num_steps] [--oracle]

``--oracle`` runs the same caller code on the CPU oracle (the test seam of ``api.py``).
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from diffusionmcmctools_amd import BiBlock, SamplingPair, accpt_rate, ll_of_accepted, loglikhd  # noqa: E402
from diffusionmcmctools_amd.models import (FitzHughNagumoAux, setup_time_grids,  # noqa: E402
                                           standard_guid_prop_time_transf)


def smoothing_estimate(AuxLaw, recording, dt, ρ=0.5, num_steps=10 ** 4, burn_in=None, every=10,
                       log=None):
    """``simple_smoothing`` of the tutorial with the estimate formed on the device.  Returns
    ``(mean, std, n, state)``: per segment the (npts × d) posterior mean path and pointwise
    standard deviation over the ``n`` recorded iterations (every ``every``-th after
    ``burn_in``, default a fifth of the run)."""
    burn_in = num_steps // 5 if burn_in is None else burn_in
    tts = setup_time_grids(recording, dt, standard_guid_prop_time_transf)
    sp = SamplingPair(AuxLaw, recording, tts)
    bb = BiBlock(sp, range(0, len(recording.obs)), ρ, True, num_steps)
    loglikhd(bb)

    se = sp.se
    se.reserve_path_moments()
    se.path_moments_every(every, burn_in=burn_in)

    # the tutorial's loop, a hundred iterations per call: draw, accept / reject, and — inside
    # the run — the accumulation of every due iteration
    for i0 in range(1, num_steps + 1, 100):
        n = min(100, num_steps - i0 + 1)
        bb.mcmc_run(i0, n)
        i = i0 + n - 1
        if log is not None and n == 100:
            log(f"{i}. ll={ll_of_accepted(bb, i)}, acceptance rate: "
                f"{accpt_rate(bb, range(i - 99, i + 1))}")

    if every == 0:  # moments off: the chain alone
        return None, None, 0, dict(sp=sp, bb=bb)
    mean, var, n = se.path_moments()
    return mean[0], [np.sqrt(v) for v in var[0]], n, dict(sp=sp, bb=bb)


def main(argv):
    import reference_tutorials as T
    num_steps = int(argv[0]) if argv and argv[0].isdigit() else 2000
    recording = T.preamble_recordings()

    def run():
        return smoothing_estimate(FitzHughNagumoAux, recording, 0.001, ρ=0.96,
                                  num_steps=num_steps, log=print)
    if "--oracle" in argv:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle as orc
        from diffusionmcmctools_amd.api import engine_override
        with engine_override(lambda model, n_points, prec, seed: orc.OracleEnsemble(
                model.kind, model.d, model.m, n_points, prec=prec, seed=seed)):
            mean, std, n, _ = run()
    else:
        mean, std, n, _ = run()
    m, s = np.concatenate(mean), np.concatenate(std)
    print(f"{n} recorded iterations; posterior mean path over {len(m)} points: "
          f"x1 in [{m[:, 0].min():.3f}, {m[:, 0].max():.3f}], "
          f"mean pointwise std (x1, x2) = ({s[:, 0].mean():.4f}, {s[:, 1].mean():.4f})")


if __name__ == "__main__":
    main(sys.argv[1:])
