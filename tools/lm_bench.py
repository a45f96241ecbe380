"""DESIGN.md 5.5b's timing table: python tools/lm_bench.py (MI355X).

pa_trajectory_lm_solve against a host-driven loop of the one-step API
(linearize, gn_step, retract, linearize, D2H of err, decision on the host), max_iters = 10,
rel_tol = abs_tol = 0 so that both run all 10 iterations on every trajectory."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import lm_ref
from perseus_amd import pipeline, synth

SIG = lm_ref.SIGMAS
KW = dict(dt=lm_ref.DT, proj_sigmas=[SIG["proj"]] * 2, dyn_sigmas=[SIG["dyn"]] * 6, cv_sigmas=[SIG["cv"]] * 3)
dev = torch.device("cuda")
ITERS = 10


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def bench(T, L, reps):
    t0 = time.time()
    pr = lm_ref.problem(T, L, 0.8)
    print(f"--- T = {T}, L = {L} (problem built in {time.time() - t0:.1f} s)", flush=True)
    y = torch.as_tensor(pr["y"], device=dev)
    init = {k: torch.as_tensor(pr[k], device=dev) for k in ("pose", "vel", "angvel")}
    x = {k: v.clone() for k, v in init.items()}
    xt = {k: v.clone() for k, v in init.items()}
    a, lin = pipeline.prepare_trajectories(y, x["pose"], x["vel"], x["angvel"], synth.CUBE_CORNERS, synth.CAMERA_K,
                                           T=T, L=L, **KW)
    assert lin["_keep"][1].data_ptr() == x["pose"].data_ptr()

    def reset():
        for k in x:
            x[k].copy_(init[k])

    res = {}
    for name, params in (("tol 0 (10 iterations on every trajectory)", dict(rel_tol=0.0, abs_tol=0.0)),
                         ("default tolerances (early exit)", {})):
        plan = pipeline.LMPlan(a, lin, T=T, L=L, **dict(lm_ref.PARAMS, max_iters=ITERS, **params))

        def dev_solve():
            reset()
            plan.launch()

        med, lo, hi = timed(dev_solve, reps)
        it = plan.out["iters"].cpu().numpy()
        print(f"device solve, eager, {name}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}), "
              f"{1 + 2 * ITERS} launches; iters min {it.min()} max {it.max()} mean {it.mean():.2f}", flush=True)
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            plan.launch()

        def dev_graph():
            reset()
            g.replay()

        med, lo, hi = timed(dev_graph, reps)
        print(f"device solve, graph replay, {name}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
        res[name] = plan.out["cost"].cpu().numpy().copy()

    # the host-driven loop over the one-step API
    at, lint = pipeline.prepare_trajectories(y, xt["pose"], xt["vel"], xt["angvel"], synth.CUBE_CORNERS,
                                             synth.CAMERA_K, T=T, L=L, **KW)
    gn = pipeline.GNPlan(lin, T=T, L=L, lam=1e-3)
    win_t = {k: v.view(T, L, -1) for k, v in xt.items()}
    nk = y.shape[1] // 2

    def cost_host(l):
        ep = l["err_proj"].cpu().numpy().reshape(T, -1)
        st = l["status"].cpu().numpy().reshape(T, -1)
        ed = l["err_dyn"].cpu().numpy().reshape(T, -1)
        ec = l["err_cv"].cpu().numpy().reshape(T, -1)
        return np.where(st == 0, ep, 0.0).sum(1) + ed.sum(1) + ec.sum(1)

    launches = [0]

    def host_loop():
        reset()
        pipeline.launch(a, dev)
        C = cost_host(lin)
        lam = 1e-3
        n = 1
        for _ in range(ITERS):
            pipeline.launch(a, dev)                      # linearize at x
            gn.lam = lam
            gn.launch()                                  # one damped step (one lambda for every trajectory)
            for k in x:
                xt[k].copy_(x[k])
            pipeline.window_retract(win_t, gn.out["delta"], gn.out["info"])
            pipeline.launch(at, dev)                     # linearize at the trial state
            Cn = cost_host(lint)                         # D2H of err (synchronises)
            acc = Cn < C
            m = torch.as_tensor(np.repeat(acc, L), device=dev)[:, None]
            for k in x:
                x[k].copy_(torch.where(m, xt[k], x[k]))
            C = np.where(acc, Cn, C)
            lam = max(lam / 10.0, 1e-12) if acc.all() else lam * 10.0
            n += 4
        launches[0] = n
        return C

    med, lo, hi = timed(host_loop, reps)
    print(f"host-driven loop, {ITERS} iterations: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); "
          f"{launches[0]} library launches + per iteration 3 state copies, 3 masked selects, 4 D2H, 1 H2D, 1 sync", flush=True)
    C = host_loop()
    print("final cost: device (tol 0) median", np.median(res["tol 0 (10 iterations on every trajectory)"]),
          "host loop (shared lambda) median", np.median(C), flush=True)


print("device", torch.cuda.get_device_name(0), flush=True)
bench(3, 6, 30)
bench(1000, 24, 10)
