#!/usr/bin/env python3
"""Cost of one accumulation of the posterior path moments (dmt_moments_accumulate) next to the
snapshot pass (dmt_snapshot_take of XX, kernel k_from_planes) and to one draw, at the full size
of a BASELINE.json config ("posterior path moments").

  python scripts/moments_bench.py --config c3 --rounds 20
      runs `rounds` times: one MCMC iteration, one snapshot of XX, one accumulation; prints one
      JSON line with the HIP-event times of the draw and the accumulation (dmt_get_timing).
      Under `rocprofv3 --kernel-trace --stats -- python scripts/moments_bench.py …` the trace
      holds every kernel's own time.
  python scripts/moments_bench.py --summarise DIR --config c3
      reads the *kernel_stats.csv under DIR and prints the kernels' average times, the bytes each
      moves per element and the rates.
"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"c2": (1024, 500, 2, 8), "c3": (65536, 1000, 2, 8), "c5": (32768, 2000, 3, 4)}  # B, N, d, sizeof(T)


def elements(config):
    B, N, d, _ = SHAPES[config]
    return B * (N + 1) * d


def run(a):
    import diffusionmcmctools_amd as dmt  # noqa: F401
    from diffusionmcmctools_amd import _lib as L
    from diffusionmcmctools_amd import workloads as W
    w = {"c2": W.c2_ou2d, "c3": lambda: W.c3_fhn(T_burn=0.2), "c5": W.c5_lorenz}[a.config]()
    ens = W.load_device(w, seed=1, init_Z=False,
                        mapping=L.MAP_AUTO if a.config == "c2" else L.MAP_LANE)
    lay = 1  # W.fill's layout
    nb = w.nblocks
    ens.loglikhd(lay, L.U, 0, nb)
    ens.snapshot_reserve(1)
    ens.moments_reserve()
    it = 1
    for _ in range(3):  # warm-up of every kernel the timed rounds launch
        ens.mcmc_run(lay, 0, nb, it, 1)
        ens.snapshot_take(0, it)
        ens.moments_accumulate(it)
        it += 1
    ens.sync()
    ens.moments_reset()
    ens.set_timing(True, kernels=(L.K_DRAW, L.K_MOMENTS))
    for _ in range(a.rounds):
        ens.mcmc_run(lay, 0, nb, it, 1)
        ens.snapshot_take(0, it)
        ens.moments_accumulate(it)
        it += 1
    ens.sync()
    draw_ms, draw_n = ens.get_timing(L.K_DRAW)
    mom_ms, mom_n = ens.get_timing(L.K_MOMENTS)
    n, _ = ens.moments_state()
    ne = elements(a.config)
    out = {"config": a.config, "rounds": a.rounds, "elements": ne, "moments_n": n,
           "draw_us_event": 1e3 * draw_ms / max(draw_n, 1), "draw_launches": draw_n,
           "moments_us_event": 1e3 * mom_ms / max(mom_n, 1), "moments_launches": mom_n,
           "moments_bytes": ne * (SHAPES[a.config][3] + 32), "kernels": L.recent_kernels()}
    out["moments_TBps_event"] = out["moments_bytes"] / (out["moments_us_event"] * 1e-6) / 1e12
    print(json.dumps(out))
    ens.close()


def summarise(a):
    files = sorted(glob.glob(os.path.join(a.summarise, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {a.summarise}")
    ne, sz = elements(a.config), SHAPES[a.config][3]
    rows = []
    with open(files[-1], newline="") as f:
        for r in csv.DictReader(f):
            rows.append((r["Name"], int(r["Calls"]), float(r["AverageNs"]) * 1e-3,
                         float(r["MinNs"]) * 1e-3, float(r["MaxNs"]) * 1e-3))
    out = {"config": a.config, "source": files[-1], "elements": ne, "kernels": []}
    for name, calls, avg, mn, mx in sorted(rows, key=lambda r: -r[1] * r[2]):
        k = {"name": name[:100], "calls": calls, "avg_us": avg, "min_us": mn, "max_us": mx}
        per = sz + 32 if "k_path_moments" in name else sz + 8 if "k_from_planes<" in name else None
        if per:
            k["bytes"] = ne * per
            k["TBps_avg"] = ne * per / (avg * 1e-6) / 1e12
        out["kernels"].append(k)
    mom = [k for k in out["kernels"] if "k_path_moments" in k["name"]]
    snap = [k for k in out["kernels"] if "k_from_planes<" in k["name"]]
    if mom and snap:
        out["moments_over_snapshot_time"] = mom[0]["avg_us"] / snap[0]["avg_us"]
        out["moments_over_snapshot_rate"] = mom[0]["TBps_avg"] / snap[0]["TBps_avg"]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(SHAPES), required=True)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--summarise")
    args = ap.parse_args()
    summarise(args) if args.summarise else run(args)
