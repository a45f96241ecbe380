"""DESIGN.md "Marginal covariances" timing table: python tools/marginals_bench.py (MI355X).

pa_trajectory_marginals in its three forms (cov, cov + cross, cov_newest only) beside
pa_trajectory_gn_step (delta and info only, GNPlan's launch) on the same factors, at
1000 x 24 (config 3's shape) and 3 x 24 (the streaming window), n_kp = 8, lam = 1e-3.
Each figure: HIP events around --launches back-to-back launches of one form, divided by the
count; the forms alternate over --rounds rounds and the median round is reported (min, max
beside it), so that a drift of the box hits every form alike."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import lm_ref
from perseus_amd import pipeline, synth

SIG = lm_ref.SIGMAS
LAM = 1e-3


def per_launch_us(fn, launches):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / launches


def bench(T, L, launches, rounds):
    pr = lm_ref.problem(T, L, 0.1)
    lin = pipeline.linearize_trajectories(torch.as_tensor(pr["y"], device="cuda"), pr["pose"], pr["vel"], pr["angvel"],
                                          synth.CUBE_CORNERS, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT,
                                          proj_sigmas=[SIG["proj"]] * 2, dyn_sigmas=[SIG["dyn"]] * 6,
                                          cv_sigmas=[SIG["cv"]] * 3)
    plans = {"gn_step (delta, info)": pipeline.GNPlan(lin, T=T, L=L, lam=LAM),
             "marginals cov": pipeline.MarginalsPlan(lin, T=T, L=L, lam=LAM),
             "marginals cov + cross": pipeline.MarginalsPlan(lin, T=T, L=L, lam=LAM, cross=True),
             "marginals cov_newest only": pipeline.MarginalsPlan(lin, T=T, L=L, lam=LAM, full=False, newest=True)}
    for p in plans.values():  # warm-up: code objects, workspaces touched
        for _ in range(10):
            p.launch()
    torch.cuda.synchronize()
    for name, p in plans.items():
        assert (p.out["info"] == 0).all(), name
    ts = {name: [] for name in plans}
    for _ in range(rounds):
        for name, p in plans.items():
            ts[name].append(per_launch_us(p.launch, launches))
    res = {}
    step = float(np.median(ts["gn_step (delta, info)"]))
    print(f"--- T = {T}, L = {L}, n_kp = 8, lam = {LAM:g}: {rounds} rounds of {launches} launches", flush=True)
    for name, v in ts.items():
        med = float(np.median(v))
        res[name] = dict(median_us=med, min_us=float(min(v)), max_us=float(max(v)), ratio_to_step=med / step)
        print(f"{name:28s} median {med:8.1f} us  (min {min(v):.1f}, max {max(v):.1f})  {med / step:5.2f} x the step",
              flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    a = ap.parse_args()
    print("device", torch.cuda.get_device_name(0), flush=True)
    out = {f"{T}x{L}": bench(T, L, a.launches, a.rounds) for T, L in ((1000, 24), (3, 24))}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
