"""Safe MPC for the double pendulum (VBOC/Safe MPC/<variant>/doublependulum_class_fixedveldir.py, drivers
<variant>/2dof_sym.py; the five variants no_constraints, hard_terminal_constraints, soft_traj_constraints,
receiding_hard_constraints, parallel) on the batched solver: k_ftr<2> through vboc_mpc_solve_batch /
vboc_mpc_soft_solve_batch, the per-problem references (OCP_solve(x0, q_ref, ...)), the drop-in classes and the closed
loops.  The oracle is oracle/vboc_oracle_ft.c with nq = 2 (tests/oracle_chain.py).  The bars are the ones
tests/test_safempc.py holds the triple to.  The network: a seeded NeuralNetDIR(4, hidden, 1) - the reference's trained
model_2dof_vboc is not in the repository - with its output bias raised (BIAS) until the hard terminal row's QP is
feasible for more than 90 % of the sample and infeasible for a few states (CPU oracle: 61 to 64 of 64 solve, the row
is violated at 5 / 1 of the initial states)."""
import math
import os

import numpy as np
import pytest

import mpc_lockstep
import oracle_chain as oc

HERE = os.path.dirname(os.path.abspath(__file__))
MEAN, STD, MARGIN = np.pi, 0.5, 2.0
TF = {10: 0.01, 3: 0.003, 1: 0.001}          # N = int(1000 Tf), the class's rule (h = 1e-3)
BIAS = {300: 2.0, 8: 2.5}


def _net(hidden, bias=None):
    import torch
    from vboc_amd.learn import NeuralNetDIR
    from vboc_amd.safempc import nn_params
    torch.manual_seed(0)
    net = NeuralNetDIR(4, hidden, 1)
    with torch.no_grad():
        net.linear_relu_stack[4].bias.fill_(BIAS[hidden] if bias is None else bias)
    return nn_params(net)


def _states(N, B=64, seed=5):
    """B states in the position box, the first 16 at rest, the others with |dtheta| <= 2; the drivers' guesses (the
    state at every stage, gravity compensation there as every control)."""
    from vboc_amd.safempc import MpcSpec2, initial_guess2
    sp = MpcSpec2(TF[N])
    assert sp.N == N and abs(sp.time_step - 1e-3) < 1e-18
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 4))
    x0[:, :2] = rng.uniform(sp.thetamin, sp.thetamax, (B, 2))
    x0[16:, 2:] = rng.uniform(-2, 2, (B - 16, 2))
    xg, ug = initial_guess2(sp, x0)
    return sp, x0, xg, ug


def _soft_Zl(N, variant):
    Zl = np.zeros(N + 1)
    if variant == "soft_N":                    # Zl = 1e6 on stage N
        Zl[N] = 1e6
    else:                                      # soft_mid: 1e9 on one interior stage (the parallel driver's pattern)
        Zl[N // 2] = 1e9
    return Zl


# ------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------
def test_spec_is_the_reference_ocp():
    from vboc_amd.safempc import MpcSpec2, driver_q_ref
    sp = MpcSpec2()
    assert (sp.nq, sp.Tf, sp.N, sp.time_step) == (2, 0.01, 10, 0.001)
    assert sp.W.tolist() == [1e4, 1e4, 1e-4, 1e-4, 1e-4, 1e-4] and sp.W_e.tolist() == [1e4, 1e4, 1e-4, 1e-4]
    assert sp.yref.tolist() == [np.pi, np.pi, 0, 0, 0, 0] and sp.yref_e.tolist() == [np.pi, np.pi, 0, 0]
    assert sp.xmin.tolist() == [np.pi - np.pi / 4] * 2 + [-10.0] * 2 and sp.xmax.tolist() == [np.pi + np.pi / 4] * 2 + [10.0] * 2
    assert sp.umax.tolist() == [10.0, 10.0] and sp.umin.tolist() == [-10.0, -10.0]
    assert (sp.lm, sp.tol, sp.qp_iter_max, sp.max_iter, sp.alpha_reduction, sp.alpha_min) == (1.0, 1e-2, 100, 1000, 0.3, 1e-2)
    assert sp.cost_scale == sp.time_step and MpcSpec2(cost_scale=1.0).cost_scale == 1.0
    assert (sp.g, sp.m, sp.l) == (9.81, (0.4, 0.4), (0.8, 0.8))
    q = driver_q_ref(sp)
    assert q.tolist() == [(sp.thetamax + sp.thetamin) / 2, sp.thetamax - 0.05]
    yr, yre = sp.references(q)
    assert yr.tolist() == [[q[0], q[1], 0, 0, 0, 0]] and yre.tolist() == [[q[0], q[1], 0, 0]]
    x = np.array([2.5, 3.5, 0.3, -0.2])
    assert sp.gravity_torque(x).tolist() == [9.81 * 0.8 * (0.4 + 0.4) * math.sin(2.5), 9.81 * 0.8 * 0.4 * math.sin(3.5)]


def test_row_of_the_oracle_is_the_numpy_row():
    """vboc_oracle_mpc_row with nq = 2 equals vboc_amd.safempc.nn_row to 1e-12, plain and margin-scaled: x[2:] is the
    velocity pair for the double."""
    from vboc_amd.safempc import nn_row
    P = _net(300)
    sp, x0, _, _ = _states(10, 32, seed=11)
    h = oc.mpc_row(2, x0, P, MEAN, STD, MARGIN)
    h0 = oc.mpc_row(2, x0, P, MEAN, STD, -1.0)
    for i in range(32):
        assert abs(h[i] - nn_row(P, MEAN, STD, x0[i], safety_margin=MARGIN)) < 1e-12
        assert abs(h0[i] - nn_row(P, MEAN, STD, x0[i])) < 1e-12
    assert np.abs(h0[:16] - h0[16:]).max() > 1e-3      # at rest vn = 1e-3, moving vn = |v|


def _fixture():
    from vboc_amd.safempc import MpcSpec2, halton_states2
    g = np.load(os.path.join(HERE, "golden", "mpc_drivers_2dof.npz"))
    sp = MpcSpec2()
    P = [g[f"net_{i}"].astype(np.float64) for i in range(6)]
    return g, sp, halton_states2(sp, int(g["test_num"])), P


def _oracle_loop_solve(sp, P, kind, q_ref):
    """The oracle behind simulate2_batch's solve for a driver variant."""
    from vboc_amd.safempc import soft_traj_weights2
    if kind in ("no_constraints", "hard_terminal_constraints"):
        def solve(x0, xg, ug):
            yr, yre = sp.references(np.tile(q_ref, (x0.shape[0], 1)))
            x, u, r, _ = oc.mpc_solve_batch(sp, x0, xg, ug, P if kind != "no_constraints" else None, MEAN, STD,
                                            rti=True, yref=yr, yref_e=yre)
            return dict(status=r["status"], x=x, u=u, qp_iter=r["qp_iter"])
        return solve
    Zl0 = soft_traj_weights2(sp.N) if kind == "soft_traj_constraints" else np.zeros(sp.N + 1)

    def solve(x0, xg, ug, w=None):
        w = w or {}
        yr, yre = sp.references(np.tile(q_ref, (x0.shape[0], 1)))
        soft = dict(margin=MARGIN, Zl=w.get("Zl", np.tile(Zl0, (x0.shape[0], 1))), W=w.get("W"), We=w.get("We"))
        x, u, r, _ = oc.mpc_solve_batch(sp, x0, xg, ug, P, MEAN, STD, rti=True, yref=yr, yref_e=yre, soft=soft)
        return dict(status=r["status"], x=x, u=u, qp_iter=r["qp_iter"])
    return solve


def _zl_default(sp, kind):
    from vboc_amd.safempc import soft_traj_weights2
    return soft_traj_weights2(sp.N) if kind == "soft_traj_constraints" else None


VARIANTS = ["no_constraints", "hard_terminal_constraints", "soft_traj_constraints", "receiding_hard_constraints",
            "parallel"]


@pytest.mark.parametrize("kind", VARIANTS)
def test_2dof_drivers_reproduce_the_reference_simulate(kind):
    """tests/golden/mpc_drivers_2dof.npz: the reference's own simulate(p) of the five 2dof drivers (AST-extracted, run
    on the oracle with injected failures, tests/golden/make_chain_golden.py mpc).  simulate2_batch on the same oracle -
    all initial states at once, the parallel driver's candidates in one batch - reproduces every problem's stop step
    and every state and control fed to the plant, bit for bit."""
    from vboc_amd.safempc import driver_q_ref, nn_row, simulate2_batch
    g, sp, x0, P = _fixture()
    solve = oc.with_forced_failures(_oracle_loop_solve(sp, P, kind, driver_q_ref(sp)), int(g["fail_mod"]),
                                    _zl_default(sp, kind))
    row = lambda x: nn_row(P, MEAN, STD, x, safety_margin=MARGIN)
    log = {}
    res, simX, _ = simulate2_batch(kind, solve, oc.rk4(2, 1e-3), sp, x0, tot_steps=int(g["tot_steps"]), row=row, log=log)
    np.testing.assert_array_equal(res, g[f"{kind}_res"])
    A = g[f"{kind}_applied"]
    np.testing.assert_array_equal(log["u"], A[..., 4:])
    np.testing.assert_array_equal(np.where(np.isnan(A[..., :4]), np.nan, simX[:, :A.shape[1]]), A[..., :4])
    assert 0 < (res < int(g["tot_steps"]) - 1).sum() < len(res)       # stopped and completed loops both present


def test_parallel_candidates_in_one_batch_equal_the_sequential_retry():
    from vboc_amd.safempc import (driver_q_ref, initial_guess2, nn_row, parallel_candidates,
                                  simulate_parallel_batch)
    ps, Zl = parallel_candidates(10, 7)
    assert ps == [10, 9, 8, 7] and Zl.shape == (4, 11) and all(Zl[c, p] == 1e9 and Zl[c].sum() == 1e9
                                                               for c, p in enumerate(ps))
    g, sp, x0, P = _fixture()
    solve = oc.with_forced_failures(_oracle_loop_solve(sp, P, "parallel", driver_q_ref(sp)), int(g["fail_mod"]))
    row = lambda x: nn_row(P, MEAN, STD, x, safety_margin=MARGIN)
    xg, ug = initial_guess2(sp, x0[:6])
    out = [simulate_parallel_batch(solve, oc.rk4(2, 1e-3), sp, x0[:6], xg, ug, row, tot_steps=40, sequential=s)
           for s in (False, True)]
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert out[1][2] < out[0][2]       # the retry stops at the first success; the batch solves every candidate


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
def _solver(sp, max_iter=None):
    from vboc_amd import lib
    s = lib.Solver(2, max(sp.N, 2))
    s.set_option("levenberg_marquardt", sp.lm)
    for t in ("stat", "eq", "ineq", "comp"):
        s.set_option(f"nlp_solver_tol_{t}", sp.tol)
    s.set_option("qp_solver_tol_stat", 1e-8)
    s.set_option("qp_solver_iter_max", sp.qp_iter_max)
    s.set_option("nlp_solver_max_iter", max_iter or sp.max_iter)
    return s


def _gpu(sp, P, x0, xg, ug, rti, soft=None, yref=None, yref_e=None, max_iter=None):
    import torch
    T = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")
    sf = None
    if soft is not None:
        sf = dict(margin=soft["margin"], Zl=T(np.broadcast_to(soft["Zl"], (x0.shape[0], sp.N + 1))))
    out = _solver(sp, max_iter).mpc_solve_device(sp, T(x0), T(xg), T(ug), [T(p) for p in P] if P is not None else None,
                                                 MEAN, STD, rti=rti, soft=sf, yref=T(yref), yref_e=T(yref_e))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


def _rti_bars(g, x, u, r, h, row_tol):
    """tests/test_safempc.py test_gpu_rti_matches_oracle's bars."""
    st, it = (g["status"] == r["status"]).mean(), (g["qp_iter"] == r["qp_iter"]).mean()
    ok = (g["status"] == 0) & (r["status"] == 0) & (g["qp_iter"] < 100) & (r["qp_iter"] < 100)
    du = np.abs(g["u"][ok] - u[ok]).max()
    dx = np.median(np.abs(g["x"][ok] - x[ok]).max(axis=(1, 2)))
    dh = np.abs(g["h"][ok] - h[ok]).max() if row_tol else 0.0
    print(f"status equal {st:.3f}, qp_iter equal {it:.3f}, both succeed {ok.mean():.3f}, max |du| {du:.2e}, "
          f"median |dx| {dx:.2e}, max |dh| {dh:.2e}; oracle statuses {np.bincount(r['status'])}")
    assert st >= 0.98 and it >= 0.95 and ok.mean() >= 0.9
    assert du < 1e-6 and dx < 1e-9
    if row_tol:
        assert dh < row_tol


RTI_CASES = [(10, 0, "none")] + [(10, hid, v) for hid in (300, 8) for v in ("hard", "soft_N", "soft_mid")] + \
            [(N, 0, "none") for N in (3, 1)] + [(N, 300, v) for N in (3, 1) for v in ("hard", "soft_N", "soft_mid")] + \
            [(N, 8, "hard") for N in (3, 1)]


def _variant_args(sp, hidden, variant):
    P = _net(hidden) if variant != "none" else None
    soft = dict(margin=MARGIN, Zl=_soft_Zl(sp.N, variant)) if variant.startswith("soft") else None
    return P, soft, (None if variant == "none" else (1e-6 if soft else 1e-8))


@pytest.mark.gpu
@pytest.mark.parametrize("N,hidden,variant", RTI_CASES)
def test_gpu_rti_matches_oracle(N, hidden, variant):
    """SQP_RTI of the 2dof classes on 64 states (16 at rest) at N = 10 and, Tf shortened, N = 3 and 1; hidden 300
    (the reference's, no multiple of 64) and 8 (below one wave); without the row, with the hard terminal row, with soft
    rows at Zl = 1e6 on stage N, with soft rows at Zl = 1e9 on one interior stage."""
    sp, x0, xg, ug = _states(N)
    P, soft, row_tol = _variant_args(sp, hidden, variant)
    g = _gpu(sp, P, x0, xg, ug, True, soft)
    x, u, r, h = oc.mpc_solve_batch(sp, x0, xg, ug, P, MEAN, STD, rti=True, soft=soft)
    _rti_bars(g, x, u, r, h, row_tol)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["none", "hard", "soft_N"])
def test_gpu_per_problem_references(variant):
    """OCP_solve(x0, q_ref, ...) in batched form: a different q_ref per problem, drawn in the position box, matches
    the oracle solved problem by problem at the RTI bars; with every row of yref_b equal to the host yref the result
    is bit-identical to the NULL form."""
    sp, x0, xg, ug = _states(10)
    P, soft, row_tol = _variant_args(sp, 300, variant)
    q = np.random.default_rng(17).uniform(sp.thetamin, sp.thetamax, (x0.shape[0], 2))
    yr, yre = sp.references(q)
    g = _gpu(sp, P, x0, xg, ug, True, soft, yref=yr, yref_e=yre)
    x, u, r, h = oc.mpc_solve_batch(sp, x0, xg, ug, P, MEAN, STD, rti=True, soft=soft, yref=yr, yref_e=yre)
    _rti_bars(g, x, u, r, h, row_tol)
    base = _gpu(sp, P, x0, xg, ug, True, soft)
    assert np.abs(base["u"] - g["u"]).max() > 1e-3                       # the references matter
    same = _gpu(sp, P, x0, xg, ug, True, soft, yref=np.tile(sp.yref, (64, 1)), yref_e=np.tile(sp.yref_e, (64, 1)))
    for k in ("status", "qp_iter", "x", "u", "cost", "h"):
        np.testing.assert_array_equal(same[k], base[k], err_msg=k)


@pytest.mark.gpu
def test_gpu_triple_per_problem_references():
    """The triple with yref_b / yref_e_b runs on the reference-carrying form of the kernel (k_ftr<3>), without them on
    k_ft<3, true> as before: with every row equal to the host yref the two are bit-identical, and a different reference
    per problem matches the oracle solved problem by problem at the RTI bars."""
    import torch
    import test_safempc as t3
    from vboc_amd import lib
    P = t3._net()
    sp, x0, xg, ug = t3._states(64, seed=5)
    T = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")

    def run(yref=None, yref_e=None):
        s = lib.Solver(3, sp.N)
        s.set_option("levenberg_marquardt", sp.lm)
        s.set_option("nlp_solver_tol_stat", 1e-6)
        s.set_option("qp_solver_tol_stat", 1e-8)
        out = s.mpc_solve_device(sp, T(x0), T(xg), T(ug), [T(p) for p in P], t3.MEAN, t3.STD, rti=True, yref=T(yref),
                                 yref_e=T(yref_e))
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}

    base, same = run(), run(np.tile(sp.yref, (64, 1)), np.tile(sp.yref_e, (64, 1)))
    for k in ("status", "qp_iter", "x", "u", "cost", "h"):
        np.testing.assert_array_equal(same[k], base[k], err_msg=k)
    yr = np.tile(sp.yref, (64, 1))
    yr[:, :3] = np.random.default_rng(19).uniform(sp.thetamin, sp.thetamax, (64, 3))
    g = run(yr, yr[:, :6].copy())
    x, u, r, h = oc.mpc_solve_batch(sp, x0, xg, ug, P, t3.MEAN, t3.STD, rti=True, yref=yr, yref_e=yr[:, :6])
    _rti_bars(g, x, u, r, h, 1e-8)
    assert np.abs(base["u"] - g["u"]).max() > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("with_row", [False, True])
def test_gpu_sqp_matches_oracle(with_row):
    """Full SQP of the 2dof class (tol 1e-2, levenberg_marquardt 1) with nlp_solver_max_iter cut to 150 on both sides,
    at tests/test_safempc.py test_gpu_sqp_matches_oracle's bars: status >= 98 %; cost (relative) and x_N of the
    problems with the same status on both sides, converged or at the cap: median <= 1e-9, max <= 2e-3.  The number of
    problems each status must have comes from the oracle's own count (90 % of it).  A problem whose SQP iteration
    counts differ must have the same status, 0 or 2; where both converged, two points that pass tol = 1e-2 on a QP
    Hessian >= levenberg_marquardt = 1 differ by at most 2 tol / lm, so x_N agrees to 2e-2."""
    sp, x0, xg, ug = _states(10, seed=7)
    P = _net(300) if with_row else None
    g = _gpu(sp, P, x0, xg, ug, False, max_iter=150)
    x, u, r, h = oc.mpc_solve_batch(sp, x0, xg, ug, P, MEAN, STD, rti=False, opts=oc.mpc_opts(sp, max_iter=150))
    print("statuses: gpu", np.bincount(g["status"], minlength=5), "oracle", np.bincount(r["status"], minlength=5))
    assert (g["status"] == r["status"]).mean() >= 0.98, (g["status"], r["status"])
    moved = np.flatnonzero((g["sqp_iter"] != r["sqp_iter"]) & (g["status"] == r["status"]))
    dxm = np.abs(g["x"][moved, -1] - x[moved, -1]).max(axis=1)
    print(f"{moved.size} problems with moved SQP-iteration counts, statuses {np.unique(g['status'][moved])}, "
          f"max |dx_N| {dxm.max() if moved.size else 0:.2e}")
    assert set(np.unique(g["status"][moved]).tolist()) <= {0, 2}
    assert (dxm[g["status"][moved] == 0] <= 2e-2).all(), (moved, dxm)
    for st_ in (0, 2):
        both = (g["status"] == st_) & (r["status"] == st_)
        n_ref = int((r["status"] == st_).sum())
        assert both.sum() >= int(0.9 * n_ref), (st_, both.sum(), n_ref)
        if not both.any():
            continue
        dc = np.abs(g["cost"] - r["cost"])[both] / np.abs(r["cost"][both])
        dx = np.abs(g["x"][:, -1] - x[:, -1]).max(axis=1)[both]
        print(f"status {st_}: {both.sum()} problems, cost median {np.median(dc):.2e} max {dc.max():.2e}, "
              f"x_N median {np.median(dx):.2e} max {dx.max():.2e}")
        assert np.median(dc) <= 1e-9 and dc.max() <= 2e-3, (st_, np.median(dc), dc.max())
        assert np.median(dx) <= 1e-9 and dx.max() <= 2e-3, (st_, np.median(dx), dx.max())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", VARIANTS)
def test_gpu_2dof_drivers_lockstep(kind):
    """The five 2dof closed loops (the fixture's initial states, 100 steps, the fixture's injected failures) on the GPU
    drop-in class, every step's OCP - every candidate of the parallel driver - also solved by the oracle from the same
    inputs and classified (tests/mpc_lockstep.py): no 'value', 'status' partings capped at 1 % (at least 2)."""
    from vboc_amd import lib
    from vboc_amd.safempc import OCPdoublependulumINIT, driver_q_ref, nn_row, simulate2_batch
    g, sp, x0, P = _fixture()
    q_ref = driver_q_ref(sp)
    if kind == "no_constraints":
        ocp = OCPdoublependulumINIT(True)
    elif kind == "hard_terminal_constraints":
        ocp = OCPdoublependulumINIT(True, P, MEAN, STD, MARGIN)
    else:
        ocp = OCPdoublependulumINIT(True, P, MEAN, STD, MARGIN, soft=True)
        if kind == "soft_traj_constraints":     # the driver's main block (:109-111)
            for i in range(1, ocp.N):
                ocp.ocp_solver.cost_set(i, "Zl", 1e6 * np.ones((1,)))
            ocp.ocp_solver.cost_set(ocp.N, "Zl", 1e6 * np.ones((1,)))
    gs = lambda x0_, xg_, ug_, w=None: ocp.solve_batch(x0_, xg_, ug_, weights=w, q_ref=q_ref)
    pairs, log = [], {}
    solve = oc.with_forced_failures(mpc_lockstep.lockstep_solve(gs, _oracle_loop_solve(sp, P, kind, q_ref), pairs),
                                    int(g["fail_mod"]), _zl_default(sp, kind))
    row = lambda x: ocp.nn_decisionfunction(P, MEAN, STD, MARGIN, x)
    res, _, solves = simulate2_batch(kind, solve, lambda X, U: lib.rk4_host(2, 1e-3, X, U), sp, x0,
                                     tot_steps=int(g["tot_steps"]), row=row, log=log)
    assert len(pairs) == solves
    mpc_lockstep.classify(pairs)
    dev = np.nanmax(np.abs(log["u"] - g[f"{kind}_applied"][..., 4:]), axis=(1, 2), initial=0.0)
    print(f"{kind}: stop steps as the fixture {(res == g[kind + '_res']).sum()}/{res.size}; applied controls vs the "
          f"fixture: median max |du| {np.median(dev):.2e}, {(dev < 1e-6).sum()} problems within 1e-6")
    # the drop-in batch-of-one call gives the batched call's result; the integrator drop-in is one RK4 step of 1e-3
    xg, ug = np.repeat(x0[:1, None], sp.N + 1, 1), np.zeros((1, sp.N, 2))
    st = ocp.OCP_solve(x0[0], q_ref, xg[0], ug[0])
    r1 = ocp.solve_batch(x0[:1], xg, ug, q_ref=q_ref)
    assert st == r1["status"][0] and np.array_equal(ocp.ocp_solver.get(sp.N, "x"), r1["x"][0, sp.N])
    if kind == "no_constraints":
        from vboc_amd.safempc import SYMdoublependulumINIT
        sim = SYMdoublependulumINIT(True)
        sim.acados_integrator.set("u", r1["u"][0, 0])
        sim.acados_integrator.set("x", x0[0])
        assert sim.acados_integrator.solve() == 0
        assert np.array_equal(sim.acados_integrator.get("x"), lib.rk4_host(2, 1e-3, x0[:1], r1["u"][:1, 0])[0])


@pytest.mark.gpu
def test_gpu_mpc_chain_rules():
    """The per-chain rules of vboc_mpc_solve_batch / vboc_mpc_soft_solve_batch: nq 4 refused; nq 1 allowed with
    hidden == 0 only (the row's x[2:] is empty for one link); a spec of another chain than the handle's is a VbocError
    naming both; an empty batch is a no-op on an nq 2 handle."""
    import torch
    from vboc_amd import lib
    from vboc_amd.safempc import MpcSpec, MpcSpec2
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")
    sp = MpcSpec2()
    s2 = _solver(sp)
    out = s2.mpc_solve_device(sp, T(np.zeros((0, 4))), T(np.zeros((0, 11, 4))), T(np.zeros((0, 10, 2))), rti=True)
    torch.cuda.synchronize()
    assert out["status"].numel() == 0
    sp3 = MpcSpec(1e-3, 0.01)
    with pytest.raises(lib.VbocError, match=r"spec nq = 3 .*handle nq = 2"):
        s2.mpc_solve_device(sp3, T(np.zeros((2, 6))), T(np.zeros((2, 11, 6))), T(np.zeros((2, 10, 3))), rti=True)

    class Spec(MpcSpec2):                      # the class data on another chain's widths, to reach the C checks
        def __init__(self, nq):
            super().__init__()
            self.nq = nq
            self.W, self.W_e = np.full(3 * nq, 1e-4), np.full(2 * nq, 1e-4)
            self.yref, self.yref_e = np.zeros(3 * nq), np.zeros(2 * nq)
            self.xmin, self.xmax = np.r_[np.full(nq, 2.0), np.full(nq, -10.0)], np.r_[np.full(nq, 4.0), np.full(nq, 10.0)]
            self.umin, self.umax = np.full(nq, -3.0), np.full(nq, 3.0)

    def call(nq, hidden, soft):
        sp_ = Spec(nq)
        x0 = np.tile(np.r_[np.full(nq, 3.0), np.zeros(nq)], (4, 1))
        P = [T(p) for p in _net(hidden)] if hidden else None
        if P is not None and nq != 2:          # a first layer of the chain's width
            P[0] = T(np.zeros((hidden, 2 * nq)))
        sf = dict(margin=MARGIN, Zl=T(np.zeros((4, sp_.N + 1)))) if soft else None
        out_ = lib.Solver(nq, 16).mpc_solve_device(sp_, T(x0), T(np.repeat(x0[:, None], sp_.N + 1, 1)),
                                                   T(np.zeros((4, sp_.N, nq))), P, MEAN, STD, rti=True, soft=sf)
        torch.cuda.synchronize()
        return out_["status"].cpu().numpy()

    for soft in (False, True):
        with pytest.raises(lib.VbocError, match="nq = 1, 2, 3"):
            call(4, 8, soft)
        with pytest.raises(lib.VbocError, match="hidden must be 0"):
            call(1, 8, soft)
    assert (call(1, 0, False) == 0).all()       # the pendulum's tracking OCP without a row solves
