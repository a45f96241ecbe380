"""DESIGN.md "Fixed-lag marginalization" timing table: python tools/prior_bench.py (MI355X).

pa_window_marginalize and pa_window_prior_linearize beside pa_trajectory_gn_step (delta and info
only, without and with a prior on frame 0) on the same factors, at 1000 x 24 (config 3's shape)
and 3 x 24 (the streaming window), n_kp = 8, lam = 1e-3; then the fp16 streaming tick (3 cameras,
720p RGBD, a 24-frame window) with and without marginalize=True.
Each kernel figure: HIP events around --launches back-to-back launches of one form, divided by
the count; the forms alternate over --rounds rounds and the median round is reported (min, max
beside it), so that a drift of the box hits every form alike.  The tick figure: HIP events around
--ticks graph replays on the pipeline's stream (device time per tick, no host staging), the two
pipelines alternating over the rounds in the same way."""
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


def report(title, ts, base):
    res = {}
    ref = float(np.median(ts[base]))
    print(f"--- {title}", flush=True)
    for name, v in ts.items():
        med = float(np.median(v))
        res[name] = dict(median_us=med, min_us=float(min(v)), max_us=float(max(v)), ratio=med / ref)
        print(f"{name:36s} median {med:8.1f} us  (min {min(v):.1f}, max {max(v):.1f})  {med / ref:5.2f} x {base}",
              flush=True)
    return res


def bench_kernels(T, L, launches, rounds):
    pr = lm_ref.problem(T, L, 0.1)
    a, lin = pipeline.prepare_trajectories(torch.as_tensor(pr["y"], device="cuda"), pr["pose"], pr["vel"],
                                           pr["angvel"], synth.CUBE_CORNERS, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT,
                                           proj_sigmas=[SIG["proj"]] * 2, dyn_sigmas=[SIG["dyn"]] * 6,
                                           cv_sigmas=[SIG["cv"]] * 3)
    pipeline.launch(a, lin["r_proj"].device)
    pose, vel, angvel = lin["_keep"][1:4]
    prior = pipeline.PriorPlan(T=T, L=L, device="cuda")
    gn, gnp = pipeline.GNPlan(lin, T=T, L=L, lam=LAM), pipeline.GNPlan(lin, T=T, L=L, lam=LAM, prior=prior)
    forms = {"gn_step (delta, info)": gn.launch,
             "gn_step_prior": gnp.launch,
             "prior_linearize": lambda: prior.linearize(pose, angvel, vel, frame=1),
             "marginalize (no delta)": lambda: prior.marginalize(lin, pose, angvel, vel, lam=LAM),
             "marginalize (re-centred)": lambda: prior.marginalize(lin, pose, angvel, vel, lam=LAM,
                                                                   delta=gn.out["delta"], gn_info=gn.out["info"])}
    # a real prior in the current buffers: one marginalization of the window itself
    prior.marginalize(lin, pose, angvel, vel, lam=LAM)
    prior.advance()
    for fn in forms.values():  # warm-up: code objects, workspaces touched
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    assert (gn.out["info"] == 0).all() and (gnp.out["info"] == 0).all() and (prior.minfo == 0).all()
    ts = {name: [] for name in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            ts[name].append(per_launch_us(fn, launches))
    return report(f"T = {T}, L = {L}, n_kp = 8, lam = {LAM:g}: {rounds} rounds of {launches} launches", ts,
                  "gn_step (delta, info)")


def bench_tick(ticks, rounds, window):
    from perseus_amd.detector import KeypointCNN
    from perseus_amd.streaming import StreamingPipeline

    m = KeypointCNN(num_channels=4)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synthetic_state_dict(0).items()})
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (3, 720, 1280, 3), dtype=np.uint8)
    depth = rng.uniform(0.2, 1.0, (3, 720, 1280)).astype(np.float32)
    pipes = {"tick fp16": StreamingPipeline(m, pose_window=window),
             "tick fp16, marginalize": StreamingPipeline(m, pose_window=window, marginalize=True)}
    for p in pipes.values():
        p.stage(rgb, depth)
        for _ in range(window + 5):  # past a full window: the marginalization computes a prior
            p.run()
    ts = {name: [] for name in pipes}
    for _ in range(rounds):
        for name, p in pipes.items():
            with torch.cuda.stream(p.stream):
                ts[name].append(per_launch_us(p.replay, ticks))
    res = report(f"streaming tick, 3 cameras, window {window}: {rounds} rounds of {ticks} graph replays", ts, "tick fp16")
    for p in pipes.values():
        p.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--window", type=int, default=24)
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    a = ap.parse_args()
    print("device", torch.cuda.get_device_name(0), flush=True)
    out = {f"{T}x{L}": bench_kernels(T, L, a.launches, a.rounds) for T, L in ((1000, 24), (3, 24))}
    out["tick"] = bench_tick(a.ticks, a.rounds, a.window)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
