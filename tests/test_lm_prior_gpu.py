"""pa_trajectory_lm_prior_solve / pa_window_lm_prior_solve (pipeline.lm_solve / LMPlan with prior=,
StreamingPipeline.solve_window(with_prior=True)) on the device against the numpy restatement
tests/lm_prior_ref.py:

  1. decision parity under a prior (case A: rejects and accepts; case B: the cost goes negative),
     over the decisions the reference takes with margin |C' - C| / |C| >= 1e-6;
  2. convergence on the magnitude of a negative cost;
  3. the outputs: prior.grad / err and the factor outputs at the final state, bit for bit, whichever
     factor set a trajectory stops on;
  4. bit identities: NULL prior, zero prior, T > CUs, two runs, graph replay;
  5. the prior with nvalid, newest_pending and a robust noise model;
  6. fixed lag reproduces batch, on the device;
  7. the streaming pipeline's solve_window(with_prior=True), graph beside eager.

Bars.  STATE_ATOL and HIST_RTOL are 10 x the worst deviation of the device from lm_prior_ref measured
on an MI355X over the compared cases of this file, and never above
tests/test_lm_gpu.py's 7.76e-11 and 1.9e-8:
  state      1.1e-11 absolute (pose entries and velocities of magnitude <= 1): the pending case,
             whose newest frame only its dynamics factor and the damping hold, as in the parent
             file; every other case <= 9.6e-13.  10 x that is above the parent's bar, so the
             bar is the parent's 7.76e-11.
  cost_hist  5.9e-14 relative to |C_ref| (case A); bar 5.9e-13.  (The parent's 1.9e-9 was set at the
             noise floor of exact keypoints, C ~ 1e-10; these cases carry 0.5 px of noise or a
             prior and stay at |C| >= 0.4.)
One case compares 9 entries per trajectory at another bar, from the reference's own error: the angular
velocities of a partly filled window's interior unmeasured frames, see test_prior_with_a_partly_filled_window.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import lm_prior_ref as R  # tests/ is on sys.path (rootdir conftest)
import lm_ref
import prior_ref
import robust_ref
from perseus_amd import _lib, pipeline, synth

pytestmark = pytest.mark.gpu

MARGIN = 1e-6  # decisions the reference takes with a smaller |C' - C| / |C| are not compared
MEASURED_STATE, MEASURED_HIST = 1.1e-11, 5.9e-14
STATE_ATOL = min(10 * MEASURED_STATE, 7.76e-11)  # (tests/test_lm_gpu.py's STATE_ATOL caps it)
HIST_RTOL = min(10 * MEASURED_HIST, 1.9e-8)
SIG = lm_ref.SIGMAS
SIGMAS = dict(proj_sigmas=[SIG["proj"]] * 2, dyn_sigmas=[SIG["dyn"]] * 6, cv_sigmas=[SIG["cv"]] * 3)
OUT = ("cost0", "cost", "iters", "status", "lambda", "cost_hist")


# ---------------------------------------------------------------- helpers
def _plan(priors, T, L):
    """A pipeline.PriorPlan holding `priors` (a list of T lm_prior_ref priors) as its current prior."""
    plan = pipeline.PriorPlan(T=T, L=L, device="cuda")
    for k, v in R.stack_priors(priors).items():
        plan.cur[k].copy_(torch.as_tensor(v))
    return plan


def _dev(pr, T, L, params, priors=None, nvalid=None, pending=False, corners=None, robust=None):
    """pipeline.lm_solve on a lm_ref problem with the priors on frame 0; numpy outputs, and
    lin / plan (the factor outputs and the PriorPlan, on the device)."""
    nv = None if nvalid is None else torch.as_tensor(np.asarray(nvalid, np.int32), device="cuda")
    plan = None if priors is None else _plan(priors, T, L)
    out = pipeline.lm_solve(torch.as_tensor(pr["y"], device="cuda"), pr["pose"], pr["vel"], pr["angvel"],
                            synth.CUBE_CORNERS if corners is None else corners, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT,
                            nvalid=nv, newest_pending=pending, proj_robust=robust, prior=plan, **SIGMAS, **params)
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy() for k in ("pose", "vel", "angvel", *OUT)}
    res.update(lin=out["lin"], plan=plan, dev_state=(out["pose"], out["vel"], out["angvel"]))
    if plan is not None:
        res.update(grad=plan.grad.cpu().numpy(), err=plan.err.cpu().numpy())
    return res


def _ref(pr, T, L, params, priors=None, nvalid=None, pending=False, corners=None, robust=None):
    with robust_ref.substituted(robust):
        return R.solve(pr["y"], pr["pose"], pr["vel"], pr["angvel"], T, L, params, priors=priors, nvalid=nvalid,
                       pending=pending, corners=corners)


def _deviation(dev, ref, free=None):
    """(state deviation, cost_hist deviation relative to |C_ref|, deviation of the angvel rows in the
    mask `free`) over every compared entry; the state deviation leaves those rows out."""
    dw = np.abs(dev["angvel"] - ref["angvel"])
    df = 0.0
    if free is not None:
        df, dw = dw[free].max(), dw[~free]
    ds = max(np.abs(dev["pose"] - ref["pose"]).max(), np.abs(dev["vel"] - ref["vel"]).max(), dw.max())
    h, g = dev["cost_hist"], ref["cost_hist"]
    np.testing.assert_array_equal(np.isnan(h), np.isnan(g))
    ok = ~np.isnan(g)
    return ds, (np.abs(h[ok] - g[ok]) / np.abs(g[ok])).max(), df


def _assert_matches(dev, ref, T, what, free=None):
    """free = (mask over the T*L frames, bar): the angvel rows in the mask are compared at that bar
    (_free_angvel), every other state entry at STATE_ATOL."""
    np.testing.assert_array_equal(dev["iters"], ref["iters"], err_msg=what)
    np.testing.assert_array_equal(dev["status"], ref["status"], err_msg=what)
    np.testing.assert_array_equal(dev["lambda"], ref["lambda"], err_msg=what)  # powers of 10, the same operations
    ds, dh, df = _deviation(dev, ref, None if free is None else free[0])
    print(f"{what}: state deviation {ds:.3g}, cost_hist relative deviation {dh:.3g}")
    assert ds <= STATE_ATOL and dh <= HIST_RTOL, (what, ds, dh)
    if free is not None:
        print(f"{what}: angvel of the unmeasured frames: deviation {df:.3g}, bar {free[1]:.3g}")
        assert df <= free[1], (what, df, free[1])
    for t in range(T):
        k = ref["iters"][t]
        assert dev["cost0"][t] == dev["cost_hist"][t, 0] and dev["cost"][t] == dev["cost_hist"][t, k]
    if "grad" in ref and "grad" in dev:  # the prior's outputs, against the reference at its final state
        sg = np.abs(ref["grad"]).max(1, keepdims=True) + 1.0
        dg = (np.abs(dev["grad"] - ref["grad"]) / sg).max()
        de = (np.abs(dev["err"] - ref["err"]) / (np.abs(ref["err"]) + 1.0)).max()
        print(f"{what}: prior grad deviation {dg:.3g} (of the largest entry), err {de:.3g}")
        assert dg <= 1e-9 and de <= 1e-9, (what, dg, de)  # tests/test_prior_gpu.py's bar for the prior's blocks


def _one(res, t, L, drop):
    return {k: (v[t * L:(t + 1) * L] if k in ("pose", "vel", "angvel") else v[t:t + 1])
            for k, v in res.items() if k not in drop}


def _well_defined(ref, T):
    """Per trajectory the number of leading iterations whose decision has margin >= MARGIN."""
    n = []
    for t in range(T):
        m = [r["margin"] >= MARGIN for r in ref["log"][t]]
        n.append(m.index(False) if False in m else len(m))
    return n


def _free_angvel(ref, pr, priors, T, L, params, frames, kw):
    """(mask, bar) of the angvel rows of each trajectory's frames[0] <= l < frames[1]: 10 x the reference's
    own error on them (lm_prior_ref.own_error of the solve `ref`), not below STATE_ATOL.  Asserts
    that everywhere else the reference is defined to STATE_ATOL."""
    with robust_ref.substituted(kw.get("robust")):
        own = R.own_error(ref, pr["y"], pr["pose"], pr["vel"], pr["angvel"], T, L, params, priors=priors,
                          **{k: v for k, v in kw.items() if k != "robust"})
    mask = (np.arange(T * L) % L >= frames[0]) & (np.arange(T * L) % L < frames[1])
    rest = max(own["pose"].max(), own["vel"].max(), own["angvel"][~mask].max())
    print(f"the reference's own error: {own['angvel'][mask].max():.3g} on the angvel of the unmeasured frames, "
          f"{rest:.3g} elsewhere (pose {own['pose'].max():.3g}, vel {own['vel'].max():.3g})")
    assert rest <= STATE_ATOL
    return mask, max(STATE_ATOL, 10 * own["angvel"][mask].max())


def _check_decisions(pr, priors, T, L, params=R.PARITY, least=5, need_reject=True, free_angvel=None, **kw):
    """tests/test_lm_gpu.py's _check_decisions with the priors: cost_hist and the accept / reject
    pattern per trajectory over its leading decisions of margin >= MARGIN, then a second solve of as
    many iterations as EVERY trajectory decides with that margin compared in full (iters, status,
    lambda, cost_hist, the final state, the prior's grad / err), and the long solve in full for the
    trajectories decided with the margin throughout.  free_angvel = (a, b): the angvel of each
    trajectory's frames a <= l < b is compared at _free_angvel's bar; every other state entry keeps
    STATE_ATOL."""
    ref = _ref(pr, T, L, params, priors, **kw)
    nok = _well_defined(ref, T)
    dec = [[r["accept"] for r in log] for log in ref["log"]]
    print("reference decisions:", dec, "well defined:", nok)
    assert min(nok) >= least
    if need_reject:
        assert any(not a for d, n in zip(dec, nok) for a in d[:n]), "no reject among the compared decisions"
    assert any(a for d, n in zip(dec, nok) for a in d[:n]), "no accept among the compared decisions"
    dev = _dev(pr, T, L, params, priors, **kw)
    for t in range(T):
        n = nok[t]
        h, g = dev["cost_hist"][t, :n + 1], ref["cost_hist"][t, :n + 1]
        dh = (np.abs(h - g) / np.abs(g)).max()
        print(f"trajectory {t}: {n} iterations compared, cost_hist relative deviation {dh:.3g}")
        assert dh <= HIST_RTOL, (t, dh)
        np.testing.assert_array_equal(np.diff(h) < 0, dec[t][:n])  # the same accepts and rejects
    m = min(nok)
    compared = False
    if m < max(len(log) for log in ref["log"]):
        short = dict(params, max_iters=m)
        ref_m = _ref(pr, T, L, short, priors, **kw)
        for t in range(T):
            assert all(r["margin"] >= MARGIN for r in ref_m["log"][t])  # every compared decision, on the reference alone
        free = _free_angvel(ref_m, pr, priors, T, L, short, free_angvel, kw) if free_angvel else None
        _assert_matches(_dev(pr, T, L, short, priors, **kw), ref_m, T, f"T={T} L={L}, {m} iterations", free)
        compared = True
    full = [t for t in range(T) if nok[t] == len(ref["log"][t])]
    free = _free_angvel(ref, pr, priors, T, L, params, free_angvel, kw) if free_angvel and full else None
    for t in full:
        _assert_matches(_one(dev, t, L, ("lin", "plan", "dev_state")), _one(ref, t, L, ("log",)), 1,
                        f"T={T} L={L}, trajectory {t}, in full",
                        None if free is None else (free[0][t * L:(t + 1) * L], free[1]))
    assert compared or len(full) == T  # a final state is compared on every path
    return dev, ref


def _cases(which, seeds=R.SEEDS, L=6):
    return R.stacked([R.case(which, s, L) for s in seeds])


# ---------------------------------------------------------------- 1. decision parity
def test_decisions_match_reference_case_a():
    """Case A, T = 3 (seeds 5, 6, 7), L = 6: 4 / 6 / 5 rejected steps, then accepts, every decision
    with margin >= 6.7e-3."""
    pr, priors = _cases("A")
    _check_decisions(pr, priors, 3, 6, least=8)


def test_decisions_match_reference_case_b_negative_cost():
    """Case B: the cost goes from ~ 9e3 through 0 to ~ -7e2; the first four decisions are taken with
    the margin (the fourth: 2.9e-3 / 5.1e-5 / 1.2e-3), all of them accepts."""
    pr, priors = _cases("B")
    dev, ref = _check_decisions(pr, priors, 3, 6, least=4, need_reject=False)
    assert (ref["cost_hist"][:, 4] < 0).all() and (dev["cost_hist"][:, 4] < 0).all()


def test_decisions_match_reference_long_window():
    """Case A at T = 2 (seeds 5, 6), L = 24."""
    pr, priors = _cases("A", (5, 6), 24)
    _check_decisions(pr, priors, 2, 24)


def test_decisions_match_reference_five_keypoints():
    """Case A with n_kp = 5 (the first five cube corners): lm_step_kernel's general instantiation."""
    pr, priors = _cases("A", (5, 6))
    pr["y"] = np.ascontiguousarray(pr["y"][:, :10])
    _check_decisions(pr, priors, 2, 6, corners=synth.CUBE_CORNERS[:5])


# ---------------------------------------------------------------- 2. negative-cost convergence
def test_converges_on_the_magnitude_of_a_negative_cost():
    """Case B, seed 6, rel_tol = 1e-3: CONVERGED at the reference's iteration (4) with cost < 0; with
    rel_tol * C in place of rel_tol * |C| the tolerance would be negative there and no accepted step
    could meet it (tests/test_lm_prior_ref.py shows that on the reference)."""
    pr, prior = R.case("B", 6)
    params = dict(R.PARITY, rel_tol=1e-3)
    ref = _ref(pr, 1, 6, params, [prior])
    assert ref["status"][0] == R.CONVERGED and ref["iters"][0] == 4 and ref["cost"][0] < 0
    assert all(r["margin"] >= MARGIN for r in ref["log"][0])
    dev = _dev(pr, 1, 6, params, [prior])
    assert dev["status"][0] == _lib.LM_CONVERGED and dev["iters"][0] == 4 and dev["cost"][0] < 0, dev
    _assert_matches(dev, ref, 1, "case B, seed 6, rel_tol 1e-3")


# ---------------------------------------------------------------- 3. outputs
def _fresh_linearize(pr, dev, T, L):
    return pipeline.linearize_trajectories(torch.as_tensor(pr["y"], device="cuda"), dev["pose"], dev["vel"],
                                           dev["angvel"], synth.CUBE_CORNERS, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT,
                                           **SIGMAS)


def test_outputs_hold_the_final_state_whichever_set_is_current():
    """Case A under PARITY: 4 / 2 / 3 accepted steps, so trajectories 0 and 1 stop with factor set
    0 (the caller's buffers) current and trajectory 2 with set 1 (the workspace's, copied out at the
    stop).  On every one: prior.grad / err are pa_window_prior_linearize(frame 0) at the final
    state and the factor outputs pa_trajectory_linearize there, bit for bit."""
    T, L = 3, 6
    pr, priors = _cases("A")
    dev = _dev(pr, T, L, R.PARITY, priors)
    accepts = (np.diff(dev["cost_hist"], axis=1) < 0).sum(1)
    print("accepted steps per trajectory:", accepts)
    assert (accepts % 2 == 0).any() and (accepts % 2 == 1).any()  # both sets end current
    fresh = _plan(priors, T, L)
    P, V, W = dev["dev_state"]
    fresh.linearize(P, W, V, frame=0)
    torch.cuda.synchronize()
    assert torch.equal(dev["plan"].grad, fresh.grad) and torch.equal(dev["plan"].err, fresh.err)
    assert dev["plan"].grad.abs().max().item() > 0
    lin = _fresh_linearize(pr, dev, T, L)
    n = 0
    for k, v in lin.items():
        if isinstance(v, torch.Tensor):
            got = dev["lin"][k].transpose(1, 2) if k.startswith("j_") else dev["lin"][k]
            assert torch.equal(got, v), k
            n += 1
    assert n >= 14


# ---------------------------------------------------------------- 4. bit identities
def _assert_same_bits(a, b, ta, tb, L, what):
    for k in ("pose", "vel", "angvel"):
        np.testing.assert_array_equal(a[k][ta * L:(ta + 1) * L], b[k][tb * L:(tb + 1) * L], err_msg=f"{what} {k}")
    for k in OUT:
        np.testing.assert_array_equal(a[k][ta], b[k][tb], err_msg=f"{what} {k}")


def _assert_same_lin(a, b):
    for k, v in a.items():
        if isinstance(v, torch.Tensor) and k != "_keep":
            assert torch.equal(v, b[k]), k


def _null_prior_call(pr, T, L, params, window):
    """pa_trajectory_lm_prior_solve / pa_window_lm_prior_solve(newest_pending = 0) with prior = NULL
    and the PARENT's workspace size, on an LMPlan's buffers."""
    dev = torch.device("cuda")
    y = torch.as_tensor(pr["y"], device=dev)
    P, V, W = (torch.as_tensor(pr[k], device=dev).clone() for k in ("pose", "vel", "angvel"))
    args, lin = pipeline.prepare_trajectories(y, P, V, W, synth.CUBE_CORNERS, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT,
                                              **SIGMAS)
    plan = pipeline.LMPlan(args, lin, T=T, L=L, **params)
    assert plan.ws.numel() == _lib.lib().pa_trajectory_lm_workspace(T, L, 8, plan.max_iters)
    o, p = plan.out, _lib.ptr
    tail = (p(o["cost0"]), p(o["cost"]), p(o["iters"]), p(o["status"]), p(o["lambda"]), p(o["cost_hist"]), p(plan.ws),
            plan.ws.numel(), _lib.stream_of(dev))
    if window:
        _lib.check(_lib.lib().pa_window_lm_prior_solve(C.byref(args), C.byref(plan.params), 0, None, *tail))
    else:
        _lib.check(_lib.lib().pa_trajectory_lm_prior_solve(C.byref(args), C.byref(plan.params), None, *tail))
    torch.cuda.synchronize()
    res = {k: o[k].cpu().numpy() for k in OUT}
    res.update(pose=P.cpu().numpy(), vel=V.cpu().numpy(), angvel=W.cpu().numpy(), lin=lin)
    return res


def test_null_and_zero_prior_are_the_parent_bit_for_bit():
    T, L = 3, 6
    pr = lm_ref.problem(T, L, 0.8)
    parent = _dev(pr, T, L, lm_ref.PARAMS)
    assert (parent["status"] == _lib.LM_CONVERGED).all()
    for window in (False, True):
        null = _null_prior_call(pr, T, L, lm_ref.PARAMS, window)
        for t in range(T):
            _assert_same_bits(null, parent, t, t, L, "NULL prior")
        _assert_same_lin(parent["lin"], null["lin"])
    zero = _dev(pr, T, L, lm_ref.PARAMS, [R.zero_prior()] * T)
    for t in range(T):
        _assert_same_bits(zero, parent, t, t, L, "zero prior")
    _assert_same_lin(parent["lin"], zero["lin"])
    assert not zero["grad"].any() and not zero["err"].any()


def _slice(pr, t, L):
    return {k: v[t * L:(t + 1) * L] for k, v in pr.items()}


def test_more_trajectories_than_cus_with_distinct_priors():
    """T = CUs + 1, L = 3, another prior on every trajectory: trajectory T - 1 is bit for bit its
    T = 1 solve (outputs, state, the prior's grad and err)."""
    T, L = torch.cuda.get_device_properties(0).multi_processor_count + 1, 3
    pr = lm_ref.problem(T, L, 0.1)
    rng = np.random.default_rng(31)
    info, eta = prior_ref.random_spd(rng, T, 10.0)
    truth0 = pr["truth"].reshape(T, L, 12)[:, 0]
    priors = [dict(R.zero_prior(), info=info[t], eta=0.01 * eta[t], xbar_pose=truth0[t].copy()) for t in range(T)]
    dev = _dev(pr, T, L, lm_ref.PARAMS, priors)
    # (exact keypoints: a few trajectories reach the rounding floor of their cost and reject steps
    # there until lambda_max, STALLED, as the solve without a prior does at that floor)
    assert np.isin(dev["status"], (_lib.LM_CONVERGED, _lib.LM_STALLED)).all(), np.unique(dev["status"], return_counts=True)
    assert (dev["status"] == _lib.LM_CONVERGED).sum() > T // 2 and (dev["cost"] <= dev["cost0"]).all()
    one = _dev(_slice(pr, T - 1, L), 1, L, lm_ref.PARAMS, priors[T - 1:])
    _assert_same_bits(dev, one, T - 1, 0, L, f"trajectory {T - 1}")
    np.testing.assert_array_equal(dev["grad"][T - 1], one["grad"][0])
    np.testing.assert_array_equal(dev["err"][T - 1], one["err"][0])
    other = _dev(_slice(pr, T - 1, L), 1, L, lm_ref.PARAMS, priors[:1])  # and the prior is this trajectory's own
    assert not np.array_equal(other["pose"], one["pose"])


def test_deterministic_and_graph_replay():
    T, L = 3, 6
    (pa, qa), (pb, qb) = _cases("A"), _cases("B", (8, 9, 10))
    a1, a2 = _dev(pa, T, L, lm_ref.PARAMS, qa), _dev(pa, T, L, lm_ref.PARAMS, qa)
    for t in range(T):
        _assert_same_bits(a1, a2, t, t, L, "two eager runs")
    np.testing.assert_array_equal(a1["grad"], a2["grad"])
    eager_b = _dev(pb, T, L, lm_ref.PARAMS, qb)
    # a plan over persistent tensors, captured once, replayed on re-seeded inputs and priors
    dev = torch.device("cuda")
    y = torch.as_tensor(pa["y"], device=dev)
    P, V, W = (torch.as_tensor(pa[k], device=dev) for k in ("pose", "vel", "angvel"))
    args, lin = pipeline.prepare_trajectories(y, P, V, W, synth.CUBE_CORNERS, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT,
                                              **SIGMAS)
    assert lin["_keep"][1].data_ptr() == P.data_ptr()  # solved in place
    prior = pipeline.PriorPlan(T=T, L=L, device=dev)
    plan = pipeline.LMPlan(args, lin, T=T, L=L, prior=prior, **lm_ref.PARAMS)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.launch()
    for src, pri, want in ((pa, qa, a1), (pb, qb, eager_b), (pa, qa, a1)):
        y.copy_(torch.as_tensor(src["y"]))
        for t_, k in ((P, "pose"), (V, "vel"), (W, "angvel")):
            t_.copy_(torch.as_tensor(src[k]))
        for k, v in R.stack_priors(pri).items():
            prior.cur[k].copy_(torch.as_tensor(v))
        g.replay()
        torch.cuda.synchronize()
        got = {k: plan.out[k].cpu().numpy() for k in plan.out}
        got.update(pose=P.cpu().numpy(), vel=V.cpu().numpy(), angvel=W.cpu().numpy())
        for t in range(T):
            _assert_same_bits(got, want, t, t, L, "graph replay")
        np.testing.assert_array_equal(prior.grad.cpu().numpy(), want["grad"])
        np.testing.assert_array_equal(prior.err.cpu().numpy(), want["err"])


# ---------------------------------------------------------------- 5. the parent's options under a prior
def _truth_priors(pr, T, L, seed, scale=10.0):
    """Per trajectory a random SPD Lambda (prior_ref.random_spd), eta = 0, xbar = the true frame 0 at rest."""
    rng = np.random.default_rng(seed)
    info, _ = prior_ref.random_spd(rng, T, scale)
    truth0 = pr["truth"].reshape(T, L, 12)[:, 0]
    return [dict(R.zero_prior(), info=info[t], xbar_pose=truth0[t].copy()) for t in range(T)]


def _noisy_problem(T, L, rot, seed=41):
    pr, _ = R.noisy(lm_ref.problem(T, L, rot), seed)
    return pr


def test_prior_with_a_partly_filled_window():
    """nvalid = 2 of 6: frames 0-3 carry no projection factor, so frame 0 is held by the prior and
    the dynamics chain alone, and 9 of the 21 rotational unknowns of frames 0-3 (the rotations of
    frames 1-3 and four angular velocities against 12 dynamics rows) by the damping alone.  The
    angular velocities of the interior unmeasured frames 1-3, which the cost sees only through
    dt w = w / 30, are where that shows: the reference itself is defined only to 2.1e-10, 1.7e-10
    and 2.2e-10 on them (the same numpy solve with its unknowns in reverse order; the angvel of
    frames 0, 4, 5: 2e-17, 3e-14, 0; poses 8.6e-12; vel 4e-15; the cost 1e-14), and the device
    measured 2.24e-10 from it on an MI355X with cost_hist at 1.8e-14.  Those 9 angvel entries per
    trajectory are compared at 10 x the reference's own error on them, computed here; every pose,
    every vel, the angvel of frames 0, 4 and 5, cost_hist, decisions, iters, status and lambda keep
    the file's bars."""
    T, L = 3, 6
    pr = _noisy_problem(T, L, 0.1)
    priors = _truth_priors(pr, T, L, 42)
    dev, _ = _check_decisions(pr, priors, T, L, lm_ref.PARAMS, least=2, need_reject=False, free_angvel=(1, L - 2),
                              nvalid=[2, 2, 2])
    st = dev["lin"]["status"].cpu().numpy().reshape(T, L, -1)
    assert (st[:, :L - 2] == 2).all() and (st[:, L - 2:] == 0).all()


def test_prior_with_the_newest_frame_pending():
    """pa_window_lm_prior_solve(newest_pending): frame L-1's projection factors carry status 3 and
    stay out, whatever its keypoint slot holds."""
    T, L = 3, 6
    pr = _noisy_problem(T, L, 0.1)
    y = pr["y"].reshape(T, L, -1).copy()
    y[:, -1] = y[:, 0]  # stale: the oldest frame's keypoints
    pr["y"] = y.reshape(T * L, -1)
    priors = _truth_priors(pr, T, L, 43)
    dev, _ = _check_decisions(pr, priors, T, L, lm_ref.PARAMS, least=2, need_reject=False, pending=True)
    st = dev["lin"]["status"].cpu().numpy().reshape(T, L, -1)
    assert (st[:, -1] == 3).all() and (st[:, :-1] == 0).all()


def test_prior_with_a_robust_noise_model():
    """proj_robust = ("huber", 1.5) with corner 2 of frame 3 40 px off in x: the cost is the sum of
    the m-estimator's losses plus e_prior (lm_prior_ref with robust_ref's factors substituted)."""
    T, L = 3, 6
    pr = _noisy_problem(T, L, 0.3)
    y = pr["y"].reshape(T, L, 8, 2).copy()
    y[:, 3, 2, 0] += np.float32(40 * R.PX)
    pr["y"] = y.reshape(T * L, 16)
    priors = _truth_priors(pr, T, L, 44)
    _check_decisions(pr, priors, T, L, lm_ref.PARAMS, least=2, need_reject=False, robust=("huber", 1.5))


def test_covariance_of_a_solve_with_a_prior_includes_it():
    """lm_solve(covariance=True, prior=): the marginal covariances of the solve's final linearization
    with Lambda in frame 0's block, against the dense inverse of the device's own factors (rtol 1e-9
    of each block's largest entry, tests/test_marginals_gpu.py's and test_prior_gpu.py's bar); and the
    prior narrows frame 0 against the same factors without it."""
    from oracle import gn_ref as G

    T, L, lam = 3, 6, 1e-3
    pr, priors = _cases("A")
    plan = _plan(priors, T, L)
    out = pipeline.lm_solve(torch.as_tensor(pr["y"], device="cuda"), pr["pose"], pr["vel"], pr["angvel"],
                            synth.CUBE_CORNERS, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT, prior=plan, covariance=True,
                            cov_lambda=lam, **SIGMAS, **lm_ref.PARAMS)
    plain = pipeline.marginals(out["lin"], T=T, L=L, lam=lam)
    torch.cuda.synchronize()
    assert (out["cov_info"] == 0).all() and (plain["info"] == 0).all()
    cov = out["cov"].cpu().numpy().reshape(T, L, 12, 12)
    f = {k: (v.transpose(1, 2) if k.startswith("j_") else v).cpu().numpy() for k, v in out["lin"].items()
         if isinstance(v, torch.Tensor)}
    for t, (A, _) in enumerate(G.stack(f, T, L, 8)):
        H = A.T @ A + lam * np.eye(12 * L)
        H[:12, :12] += priors[t]["info"]
        S = np.linalg.inv(H)
        for l in range(L):
            want = S[12 * l:12 * l + 12, 12 * l:12 * l + 12]
            np.testing.assert_allclose(cov[t, l], want, rtol=1e-9, atol=1e-9 * np.abs(want).max(), err_msg=f"{t} {l}")
    d0 = np.einsum("tii->ti", cov[:, 0])
    p0 = np.einsum("tii->ti", plain["cov"].cpu().numpy().reshape(T, L, 12, 12)[:, 0])
    assert (d0 <= p0 * (1 + 1e-9)).all() and (d0 < p0 * (1 - 1e-3)).any()


# ---------------------------------------------------------------- 6. fixed lag reproduces batch
def test_fixed_lag_reproduces_batch_on_the_device():
    """tests/test_lm_prior_ref.py's construction, T = 3 (seeds 5, 6, 7), every step on the device:
    pa_trajectory_lm_solve on 7 frames -> pa_window_marginalize (lambda 0, no input prior, no
    delta) -> pa_trajectory_lm_prior_solve on frames 1..6 from 0.3 rad off lands within 1e-7 of the
    7-frame solve; the same solve without the prior stays >= 1e-3 away."""
    T, L = 3, 7
    pr7 = {k: np.concatenate([R.noisy(lm_ref.problem(1, L, 0.1, s), s + 1000)[0][k] for s in R.SEEDS])
           for k in ("y", "pose", "vel", "angvel")}
    batch = _dev(pr7, T, L, R.TIGHT)
    # (rel_tol 1e-12 is at the rounding floor of the cost: a trajectory may end there CONVERGED or,
    # every further step rejected, STALLED / MAX_ITERS; either way it stands at the minimum)
    print("7-frame solves: status", batch["status"], "iters", batch["iters"])
    m = pipeline.PriorPlan(T=T, L=L, device="cuda")
    P, V, W = batch["dev_state"]
    m.marginalize(batch["lin"], P, W, V, lam=0.0, n_kp=8)
    torch.cuda.synchronize()
    assert (m.minfo == 0).all()
    priors = [{k: m.nxt[k][t].cpu().numpy() for k in R.PRIOR_KEYS} for t in range(T)]
    for t in range(T):
        np.testing.assert_array_equal(priors[t]["xbar_pose"], batch["pose"].reshape(T, L, 12)[t, 1])
    far = {k: np.concatenate([lm_ref.problem(1, L, 0.3, s)[k] for s in R.SEEDS]) for k in ("pose", "vel", "angvel")}
    sub = {k: np.ascontiguousarray(v.reshape(T, L, -1)[:, 1:].reshape(T * (L - 1), -1))
           for k, v in dict(far, y=pr7["y"]).items()}
    with_prior = _dev(sub, T, L - 1, R.TIGHT, priors)
    without = _dev(sub, T, L - 1, R.TIGHT)
    for t in range(T):
        want = {k: batch[k].reshape(T, L, -1)[t] for k in ("pose", "vel", "angvel")}
        dw = R.distance({k: with_prior[k].reshape(T, L - 1, -1)[t] for k in want}, want)
        do = R.distance({k: without[k].reshape(T, L - 1, -1)[t] for k in want}, want)
        print(f"seed {R.SEEDS[t]}: distance from the 7-frame solve {dw:.3g} with the prior, {do:.3g} without")
        assert dw <= 1e-7 and do >= 1e-3, (t, dw, do)


# ---------------------------------------------------------------- 7. streaming
from test_streaming_pose_gpu import LW, _init, _keypoints, _model, _pipe, _truth  # noqa: E402

# The streaming solve starts at the ticks' estimate, so its last accepted step lowers a cost of order
# 1 by ~1e-7 relative: below MARGIN, which is set for the parity cases' noise floor.  A decision can
# differ from the reference's only if the two costs differ by more than its margin.  Here the cost
# is a sum of ~60 f64 terms of order 1e-2 .. 1, each a squared difference of ~128 px numbers taken at
# a 0.5 px residual: eps * 128 / 0.5 = 6e-14 relative per term.  1e-8 is five orders above that.
STREAM_MARGIN = 1e-8


@pytest.fixture(scope="module")
def model():
    return _model()


def _prior_bits(a, b, which):
    for key in R.PRIOR_KEYS:
        assert torch.equal(getattr(a.prior, which)[key], getattr(b.prior, which)[key]), (which, key)


def test_streaming_solve_window_with_prior(model):
    n, ticks = 3, LW + 2
    truth, _, _ = _truth(n, ticks + 4)
    rng = np.random.default_rng(4)
    g, e = _pipe(model, True, init=_init(n), marginalize=True), _pipe(model, False, init=_init(n), marginalize=True)
    for k in range(ticks):
        y = _keypoints(truth[k], 0.5, rng)
        (qg, ig), (qe, ie) = g.tick_keypoints(y), e.tick_keypoints(y)
        assert (ig == 0).all() and np.array_equal(qg, qe), k
    graph = g.pose_graph
    assert graph is not None
    assert g.prior.cur["info"].abs().max().item() > 0.0
    with pytest.raises(ValueError, match="marginal"):
        g.solve_window()
    plain = _pipe(model, False, init=_init(n))
    with pytest.raises(ValueError, match="marginalize=True"):
        plain.solve_window(with_prior=True)
    plain.close()
    before = g.window_state()
    priors = [{k: g.prior.cur[k][c].cpu().numpy() for k in R.PRIOR_KEYS} for c in range(n)]
    rg, re = g.solve_window(with_prior=True), e.solve_window(with_prior=True)
    print("solve_window(with_prior=True):", rg)
    assert (rg["status"] == _lib.LM_CONVERGED).all() and (rg["cost"] <= rg["cost0"]).all(), rg
    for k in rg:
        np.testing.assert_array_equal(rg[k], re[k], err_msg=k)
    after = g.window_state()
    for key, v in after.items():
        np.testing.assert_array_equal(v, e.window_state()[key], err_msg=key)
    _prior_bits(g, e, "nxt")
    assert torch.equal(g.prior.grad, e.prior.grad)
    # the solved window against the reference run from the pre-solve window and the prior's host copy
    ref = R.solve(before["y"], before["pose"].reshape(n * LW, 12), before["vel"].reshape(n * LW, 3),
                  before["angvel"].reshape(n * LW, 3), n, LW, dict(lm_ref.PARAMS, max_iters=20), priors=priors)
    print("reference decisions:", [[(r["accept"], f"{r['margin']:.2g}") for r in log] for log in ref["log"]])
    assert all(r["margin"] >= STREAM_MARGIN for log in ref["log"] for r in log)
    np.testing.assert_array_equal(rg["iters"], ref["iters"])
    np.testing.assert_array_equal(rg["status"], ref["status"])
    ds = max(np.abs(after[k].reshape(n * LW, -1) - ref[k]).max() for k in ("pose", "vel", "angvel"))
    dc = (np.abs(rg["cost"] - ref["cost"]) / np.abs(ref["cost"])).max()
    print(f"solved window: state deviation {ds:.3g}, final cost relative deviation {dc:.3g}")
    assert ds <= STATE_ATOL and dc <= HIST_RTOL, (ds, dc)
    # prior.nxt: the marginal of the device's own factors at the solved window
    f = {k: (v.transpose(1, 2) if k.startswith("j_") else v).cpu().numpy() for k, v in g.lin.items()
         if isinstance(v, torch.Tensor) and k != "_keep"}
    grad = g.prior.grad.cpu().numpy()
    info, eta, minfo = prior_ref.marginalize(f, n, LW, 8, g.gn.lam, np.stack([p["info"] for p in priors]), grad)
    assert (minfo == 0).all() and (g.prior.minfo == 0).all()
    for key, want in (("info", info), ("eta", eta)):
        got = g.prior.nxt[key].cpu().numpy()
        for c in range(n):
            np.testing.assert_allclose(got[c], want[c], rtol=0, atol=1e-9 * np.abs(want[c]).max(), err_msg=key)
    np.testing.assert_array_equal(g.prior.nxt["xbar_pose"].cpu().numpy(), after["pose"][:, 1])
    # four more ticks on the solved window: graph == eager, no recapture
    for k in range(ticks, ticks + 4):
        y = _keypoints(truth[k], 0.5, rng)
        (qg, ig), (qe, ie) = g.tick_keypoints(y), e.tick_keypoints(y)
        assert (ig == 0).all() and (g.prior.minfo == 0).all(), (k, ig)
        np.testing.assert_array_equal(qg, qe, err_msg=str(k))
    for key, v in g.window_state().items():
        np.testing.assert_array_equal(v, e.window_state()[key], err_msg=key)
    _prior_bits(g, e, "cur")
    _prior_bits(g, e, "nxt")
    assert g.pose_graph is graph
    g.close()
    e.close()
