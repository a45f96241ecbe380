"""DESIGN.md 5.5b's timing table: python tools/lm_bench.py (MI355X).

pa_trajectory_lm_solve against a host-driven loop of the one-step API
(linearize, gn_step, retract, linearize, D2H of err, decision on the host), max_iters = 10,
rel_tol = abs_tol = 0 so that both run all 10 iterations on every trajectory.

DESIGN.md 5.5f's: python tools/lm_bench.py --prior [--ab PARENT_LIB] [--rounds N]
the device solve with and without a marginalization prior on frame 0 (pa_trajectory_lm_prior_solve,
a random SPD Lambda at the true frame 0), same protocol, at 3 x 6 and 1000 x 24; with --ab also the
no-prior solve of this build against another build of the library (the parent commit's), one fresh
process per build and round, alternating on one box (PERSEUS_AMD_LIB_AB, as tools/so_ab.py)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
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


SHAPES = ((3, 6, 30), (1000, 24, 10))  # T, L, timed runs (5.5b's protocol)
TOL0 = dict(lm_ref.PARAMS, max_iters=ITERS, rel_tol=0.0, abs_tol=0.0)


def solve_times(pr, T, L, reps, with_prior):
    """{eager, graph: (median, min, max) ms} of the tol-0 device solve on problem `pr`, with a random
    SPD prior at the true frame 0 (with_prior) or through the parent entry point."""
    import prior_ref

    y = torch.as_tensor(pr["y"], device=dev)
    init = {k: torch.as_tensor(pr[k], device=dev) for k in ("pose", "vel", "angvel")}
    x = {k: v.clone() for k, v in init.items()}
    a, lin = pipeline.prepare_trajectories(y, x["pose"], x["vel"], x["angvel"], synth.CUBE_CORNERS, synth.CAMERA_K,
                                           T=T, L=L, **KW)
    prior = None
    if with_prior:
        prior = pipeline.PriorPlan(T=T, L=L, device=dev)
        info, _ = prior_ref.random_spd(np.random.default_rng(7), T, 10.0)
        prior.cur["info"].copy_(torch.as_tensor(info))
        prior.cur["xbar_pose"].copy_(torch.as_tensor(np.asarray(pr["truth"]).reshape(T, L, 12)[:, 0].copy()))
    plan = pipeline.LMPlan(a, lin, T=T, L=L, **({"prior": prior} if with_prior else {}), **TOL0)

    def reset():
        for k in x:
            x[k].copy_(init[k])

    def eager():
        reset()
        plan.launch()

    out = {"eager": timed(eager, reps)}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        plan.launch()

    def graph():
        reset()
        g.replay()

    out["graph"] = timed(graph, reps)
    out["cost"] = float(np.median(plan.out["cost"].cpu().numpy()))
    return out


def load_problems(path):
    z = np.load(path)
    return {(T, L): {k: z[f"{T}_{L}_{k}"] for k in ("y", "pose", "vel", "angvel", "truth")} for T, L, _ in SHAPES}


def prior_leg(ab, rounds):
    print("device", torch.cuda.get_device_name(0), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "problems.npz")  # built once: every child process loads them
        np.savez(path, **{f"{T}_{L}_{k}": v for T, L, _ in SHAPES for k, v in lm_ref.problem(T, L, 0.8).items()})
        prs = load_problems(path)
        for T, L, reps in SHAPES:
            for with_prior in (False, True):
                r = solve_times(prs[T, L], T, L, reps, with_prior)
                for form in ("eager", "graph"):
                    med, lo, hi = r[form]
                    print(f"T = {T}, L = {L}, {'with a prior' if with_prior else 'no prior   '}, {form}: median "
                          f"{med:.3f} ms (min {lo:.3f}, max {hi:.3f}); final cost median {r['cost']:.6g}", flush=True)
        if not ab:
            return
        libs = {"parent": os.path.abspath(ab), "this build": pipeline._lib.lib_path()}
        res = {n: [] for n in libs}
        for r in range(rounds):
            for name, lib in libs.items():
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path],
                                     env=dict(os.environ, PERSEUS_AMD_LIB_AB=lib), capture_output=True, text=True,
                                     timeout=300)
                if out.returncode != 0:
                    print(out.stdout[-2000:], out.stderr[-4000:])
                    raise SystemExit(f"child failed for {lib}")
                res[name].append(json.loads(out.stdout.strip().splitlines()[-1]))
                print(f"round {r} {name}: {res[name][-1]}", flush=True)
        for key in res["parent"][0]:
            if key.startswith("cost"):
                assert len({r[key] for rs in res.values() for r in rs}) == 1, f"{key}: the builds disagree"
                continue
            m = {n: statistics.median(r[key] for r in rs) for n, rs in res.items()}
            sp = {n: (min(r[key] for r in rs), max(r[key] for r in rs)) for n, rs in res.items()}
            print(f"no prior, {key}: parent {m['parent']:.3f} ms ({sp['parent'][0]:.3f} .. {sp['parent'][1]:.3f}), this "
                  f"build {m['this build']:.3f} ms ({sp['this build'][0]:.3f} .. {sp['this build'][1]:.3f}), ratio "
                  f"{m['this build'] / m['parent']:.3f} (medians over {rounds} alternating rounds of per-process medians)")
        print("final costs of the two builds: bit-identical")


def child(path):
    """One process on the library PERSEUS_AMD_LIB_AB names: the no-prior medians as one JSON line."""
    prs = load_problems(path)
    out = {}
    for T, L, reps in SHAPES:
        r = solve_times(prs[T, L], T, L, reps, False)
        out[f"{T}x{L} eager"] = r["eager"][0]
        out[f"{T}x{L} graph"] = r["graph"][0]
        out[f"cost {T}x{L}"] = r["cost"].hex()
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--prior", action="store_true", help="5.5f: the solve with / without a prior")
    ap.add_argument("--ab", help="with --prior: another build of the library to time the no-prior solve against")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child)
    elif args.prior:
        prior_leg(args.ab, args.rounds)
    else:
        print("device", torch.cuda.get_device_name(0), flush=True)
        bench(3, 6, 30)
        bench(1000, 24, 10)
