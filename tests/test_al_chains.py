"""The AL labelling OCP for the double pendulum and the pendulum (AL/doublependulum_class_al.py,
AL/pendulum_class_al.py; drivers AL/doublependulum_al.py, AL/pendulum_al.py): the specs against the reference classes'
data, the oracle restatement (nq-generic in oracle/vboc_oracle_ft.c, bound in tests/oracle_chain.py) pinned by the
independent LP, the batched driver against the reference's own functions (tests/golden/al_testing_chains.npz,
tests/golden/make_chain_golden.py), and the GPU solver (k_ftr<1>, k_ftr<2> through vboc_al_solve_batch)
against the oracle.

Short horizons: at N = 1 and N = 3 the oracle's interior point declares convergence on some QPs the LP proves
infeasible (5 / 96 and 2 / 96 states) - the step it returns is no solution, so it is no yardstick:
the short-horizon GPU cases draw their states on the CPU, drop those on which the oracle's label and the LP part (at most
10 % of the sample) and compare the GPU with the oracle on the rest.  At the classes' own N = 100 nothing is dropped."""
import json
import os

import numpy as np
import pytest

import oracle_chain as oc
from vboc_amd.al import AlSpec, out_of_bounds, unlabeled_states
from vboc_amd.al import testing_batch as al_testing_batch

HERE = os.path.dirname(os.path.abspath(__file__))
CAP_SHARE = 0.02


def al_spec(nq, N=100):
    """AlSpec(nq) on a horizon of N of the class's intervals (time step 0.01)."""
    spec = AlSpec(nq)
    spec.N = N
    return spec


def in_box_states(spec, n, seed, vel_scale=1.0):
    """n seeded states inside the class's box, the velocities scaled by vel_scale (short horizons: a state at full
    speed cannot come to rest in a few intervals, so every label would be 0)."""
    S = unlabeled_states(spec, 3 * n, np.random.default_rng(seed))
    S = np.array([s for s in S if not out_of_bounds(spec, s)][:n])
    S[:, spec.nq:] *= vel_scale
    return S


# (nq, N, velocity scale): N = 1 has only stage 0 and the terminal stage; N = 65 is the first horizon where the
# stage-parallel passes wrap past lane 63; N = 100 is the classes' own.  The scale is 0.02 N up to 1, except the
# pendulum at N = 1, where scaled velocities give label 1 only (checked below): the full box there.
CASES = [(2, 1, 0.02), (2, 3, 0.06), (2, 65, 1.0), (2, 100, 1.0), (1, 1, 1.0), (1, 100, 1.0)]
_cache = {}


def case_states(nq, N, scale):
    """(spec, states, oracle result) of a case: 96 drawn, those with oracle label != LP dropped for N < 100."""
    key = (nq, N)
    if key not in _cache:
        spec = al_spec(nq, N)
        S = in_box_states(spec, 96, seed=100 * nq + N, vel_scale=scale)
        r = oc.al_solve_batch(spec, S)
        dropped = 0
        if N < 100:
            feas = np.array([oc.lp_feasible(spec, s) for s in S])
            keep = (r["label"] == 1) == feas
            dropped = int((~keep).sum())
            S = np.ascontiguousarray(S[keep])
            r = {k: v[keep] for k, v in r.items()}
        _cache[key] = (spec, S, r, dropped)
    return _cache[key]


def test_al_specs_are_the_reference_classes_data():
    for nq, umax in ((1, 3.0), (2, 10.0), (3, 10.0)):
        sp = AlSpec(nq)
        assert (sp.nq, sp.nx, sp.nu, sp.N, sp.Tf, sp.time_step) == (nq, 2 * nq, nq, 100, 1.0, 0.01)
        assert sp.W.tolist() == [0.0] * nq + [2.0] * nq + [0.0] * nq and sp.W_e.tolist() == [0.0] * nq + [2.0] * nq
        assert sp.umax.tolist() == [umax] * nq and sp.umin.tolist() == [-umax] * nq
        assert sp.xmin.tolist() == [np.pi - np.pi / 4] * nq + [-10.0] * nq
        assert sp.xmax.tolist() == [np.pi + np.pi / 4] * nq + [10.0] * nq
        assert sp.xmin_e.tolist() == [np.pi - np.pi / 4] * nq + [0.0] * nq
        assert sp.xmax_e.tolist() == [np.pi + np.pi / 4] * nq + [0.0] * nq
        assert (sp.lm, sp.qp_iter_max, sp.cost_scale) == (0.0, 50, 0.01)
    d = AlSpec()                                         # the triple's, as before
    assert d.nq == 3 and AlSpec(cost_scale=1.0).cost_scale == 1.0 and AlSpec(2, 1.0).nq == 2
    with pytest.raises(ValueError):
        AlSpec(4)


@pytest.mark.parametrize("nq", [2, 1])
def test_oracle_labels_are_the_lp_feasibility_at_the_class_horizon(nq):
    """N = 100: every label equals the LP's answer, except a feasible QP at the iteration cap (at most 2 % of the
    sample - tests/test_al.py's rule; measured 0 for both chains); both labels present; a label-1 step satisfies the
    linearised QP to 1e-8."""
    spec = al_spec(nq)
    S = in_box_states(spec, 96, seed=20 + nq)
    r = oc.al_solve_batch(spec, S)
    feas = np.array([oc.lp_feasible(spec, s) for s in S])
    assert set(np.unique(r["status"])) <= {0, 4}
    capped_feasible = int(((r["qp_iter"] >= spec.qp_iter_max) & feas).sum())
    assert capped_feasible <= CAP_SHARE * len(S), capped_feasible
    wrong = np.flatnonzero((r["label"] == 1) != feas)
    assert all(feas[i] and r["qp_iter"][i] >= spec.qp_iter_max for i in wrong), wrong
    assert 0 < feas.sum() < len(S)
    for i in np.flatnonzero(r["label"] == 1):
        assert oc.step_violation(spec, S[i], r["x"][i], r["u"][i]) < 1e-8, i
    ok = r["label"] == 1
    assert np.abs(r["x"][:, 0] - S).max() == 0.0 and np.abs(r["x"][ok, -1, nq:]).max() < 1e-9


@pytest.mark.parametrize("nq,N,scale", CASES)
def test_gpu_case_samples_keep_both_labels(nq, N, scale):
    """A guard on the GPU cases' samples, not on the feature: at most 10 % dropped (oracle label != LP, at N < 100
    only), both labels left."""
    spec, S, r, dropped = case_states(nq, N, scale)
    print(f"nq {nq} N {N}: {len(S)} states, {dropped} dropped, labels 0/1/2 "
          f"{[(r['label'] == l).sum() for l in (0, 1, 2)]}")
    assert dropped <= 0.1 * 96
    assert (r["label"] == 0).any() and (r["label"] == 1).any()


# ----------------------------------------------------------------------------------------------------------------
# the drivers: testing / testing_guess of AL/doublependulum_al.py and AL/pendulum_al.py
# ----------------------------------------------------------------------------------------------------------------
def _fixture(nq):
    """(the drivers' return values {results, results_guess}, states X, in-bounds states S, their stored guess
    trajectories [len(S), N+1, 2nq]) from tests/golden/al_testing_chains.npz (layout: make_chain_golden.py)."""
    f = np.load(os.path.join(HERE, "golden", "al_testing_chains.npz"))
    X = f[f"X_{nq}"]
    g = {}
    for name, tag in (("results", ""), ("results_guess", "g")):
        trajs = iter(f[f"traj{tag}_{nq}"])
        g[name] = [None if k == 0 else ([*map(float, s0), 1, 0], None) if k == 1 else
                   ([*map(float, s0), 0, 1], next(trajs).tolist()) for s0, k in zip(X, f[f"kind{tag}_{nq}"])]
    S = np.array([s for s in X if not out_of_bounds(AlSpec(nq), s)])
    G = f[f"guess_{nq}"].astype(np.float64)
    assert G.shape == (len(S), 100, 2 * nq)
    return g, X, S, np.concatenate([S[:, None, :], G], axis=1)


def _same(got, ref, tol=0.0):
    assert len(got) == len(ref)
    for b, (a, r) in enumerate(zip(got, ref)):
        if r is None:
            assert a is None, b
            continue
        assert a[0] == r[0], b
        assert (a[1] is None) == (r[1] is None), b
        if r[1] is not None:
            assert np.abs(np.asarray(a[1]) - np.asarray(r[1])).max() <= tol, b


@pytest.mark.parametrize("nq", [2, 1])
def test_testing_batch_reproduces_the_reference_drivers_on_the_oracle(nq):
    """testing(s0) and testing_guess(s0) of the chain's driver, AST-extracted and run on the oracle
    (tests/golden/make_chain_golden.py): testing_batch on the same oracle reproduces both bit for bit.  The guess
    trajectories are stored in the fixture (the float32 values the network returned),
    so every host feeds identical inputs."""
    g, X, S, xg = _fixture(nq)
    spec = AlSpec(nq)
    fn = lambda S_: (lambda r: (r["label"], r["x"]))(oc.al_solve_batch(spec, S_))
    _same(al_testing_batch(spec, X, fn), g["results"])
    fng = lambda S_: (lambda r: (r["label"], r["x"]))(oc.al_solve_batch(spec, S_, x_guess=xg))
    _same(al_testing_batch(spec, X, fng), g["results_guess"])
    n_feas = sum(r is not None and r[0][-1] == 1 for r in g["results"])
    assert len(X) > len(S) and 0 < n_feas < len(S)


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _gpu_al(spec, S, x_guess=None):
    import torch
    from vboc_amd import lib
    s = lib.Solver(spec.nq, max(spec.N, 2))
    s.set_option("levenberg_marquardt", spec.lm)
    s.set_option("qp_solver_iter_max", spec.qp_iter_max)
    s.set_option("nlp_solver_tol_stat", 1e-6)
    s.set_option("qp_solver_tol_stat", 1e-8)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")
    out = s.al_solve_device(spec, T(S), x_guess=T(x_guess) if x_guess is not None else None)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


@pytest.mark.gpu
@pytest.mark.parametrize("nq,N,scale", CASES)
def test_gpu_labels_match_oracle(nq, N, scale):
    """tests/test_al.py's bars for the triple, on the new chains: labels equal except where one side is at the QP cap
    (at most 1 %); on problems both label 1, x within 1e-7 and u within 1e-6; QP iteration counts equal on >= 95 %.

    Two of these bars are re-derived for the short horizons from the oracle's own rounding spread
    (tests/golden/al_chain_spread.json, tools/al_chain_spread.py: the oracle under its four compiler-flag sets on these
    very states).  On an infeasible QP the interior point has nothing to converge to; whether it ends in a failed
    factorisation (label 0) or in a stop test passed on a point that is no solution (label 1), and
    after how many iterations, is decided by rounding, and the oracle parts from ITSELF there: labels on 6 / 89
    (nq 2, N 1), 3 / 93 (nq 2, N 3) and 3 / 95 (nq 1, N 1) states, none at the cap but one; iteration counts on 8, 13
    and 81 states, every one of them labelled 0.  Measured on the GPU against the committed oracle: labels part on 3,
    2 and 0 states, iteration counts on 6, 8 and 77.  The bars are counts, so DESIGN section 3's factor of 100 cannot
    apply; they are held at ONE times the oracle's own figures, on the states where it can happen at all:
      * a label may also part, away from the cap, on a state whose QP the LP proves infeasible, on at most as many
        states as the oracle's own builds part on (the fixture's labels_differ_not_at_cap);
      * where the oracle's own builds differ in their iteration counts on more than 5 % of the case, the 95 % bar is
        held on the problems that have a solution (both label 1), and over all problems the count of unequal ones is
        held to the oracle's own (the fixture's qp_iter_differ).
    At N = 65 and N = 100 the fixture shows no parted label and at most 3 / 96 iteration counts, and the bars are the
    triple's unchanged."""
    spec, S, r, _ = case_states(nq, N, scale)
    sprd = json.load(open(os.path.join(HERE, "golden", "al_chain_spread.json")))["cases"][f"nq{nq}/N{N}"]
    assert sprd["n"] == len(S)
    g = _gpu_al(spec, S)
    diff = np.flatnonzero(g["label"] != r["label"])
    print(f"nq {nq} N {N}: {len(S)} states, {len(diff)} labels part, qp_iter equal "
          f"{(g['qp_iter'] == r['qp_iter']).mean():.3f}")
    for i in diff:
        print(f"  state {i} {S[i].tolist()}: gpu label {g['label'][i]} status {g['status'][i]} qp_iter {g['qp_iter'][i]}; "
              f"oracle label {r['label'][i]} status {r['status'][i]} qp_iter {r['qp_iter'][i]}")
    at_cap = [i for i in diff if max(g["qp_iter"][i], r["qp_iter"][i]) >= spec.qp_iter_max]
    away = [i for i in diff if i not in at_cap]
    assert len(at_cap) <= 0.01 * len(S), at_cap
    assert len(away) <= sprd["labels_differ_not_at_cap"], (away, sprd)
    assert not any(oc.lp_feasible(spec, S[i]) for i in away), away
    ok = (g["label"] == 1) & (r["label"] == 1)
    assert ok.any()
    dx, du = np.abs(g["x"][ok] - r["x"][ok]).max(), np.abs(g["u"][ok] - r["u"][ok]).max()
    print(f"  max |dx| {dx:.2e}, max |du| {du:.2e} on {ok.sum()} problems")
    assert dx < 1e-7 and du < 1e-6
    same = g["qp_iter"] == r["qp_iter"]
    if sprd["qp_iter_differ"] <= 0.05 * len(S):
        assert same.mean() >= 0.95, same.mean()
    else:
        print(f"  qp_iter equal on {same[ok].mean():.3f} of the problems both label 1; unequal over all "
              f"{(~same).sum()} (the oracle's own builds: {sprd['qp_iter_differ']})")
        assert same[ok].mean() >= 0.95 and (~same).sum() <= sprd["qp_iter_differ"]


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [2, 1])
def test_gpu_dropin_compute_problem(nq):
    """compute_problem and compute_problem_nnguess of the drop-in classes on 8 states each: labels as the oracle's,
    trajectories within 1e-7; the AL driver fixtures reproduced with exact label equality and trajectories within
    1e-7 (the stored guesses make testing_guess input-identical)."""
    from vboc_amd import al
    ocp = (al.OCPdoublependulumINIT if nq == 2 else al.OCPpendulumINIT)()
    spec = ocp.spec
    assert spec.nq == nq and ocp.N == 100
    g, X, S, xg = _fixture(nq)
    r = oc.al_solve_batch(spec, S[:8])
    for i, s in enumerate(S[:8]):
        res = ocp.compute_problem(s[0], s[1]) if nq == 1 else ocp.compute_problem(s[:nq], s[nq:])
        assert res == r["label"][i]
        if res == 1:
            assert np.abs(np.array([ocp.ocp_solver.get(k, "x") for k in range(ocp.N + 1)]) - r["x"][i]).max() < 1e-7
    # compute_problem_nnguess: a guess model that returns the fixture's stored trajectory of the state - float32
    # values, which the class's FP32 pass (x * 1 + 0) returns exactly, so both sides linearise at the same points
    rg = oc.al_solve_batch(spec, S[:8], x_guess=xg[:8])
    for i, s in enumerate(S[:8]):
        model, mean, std = _StoredGuess(xg[i]), 0.0, 1.0
        res = (ocp.compute_problem_nnguess(s[0], s[1], model, mean, std) if nq == 1 else
               ocp.compute_problem_nnguess(s[:nq], s[nq:], model, mean, std))
        assert res == rg["label"][i]
        if res == 1:
            assert np.abs(ocp.ocp_solver.x - rg["x"][i]).max() < 1e-7
    # the driver fixtures
    _same(al_testing_batch(spec, X, ocp.labels), g["results"], tol=1e-7)
    fng = lambda S_: (lambda o: (o["label"], o["x"]))(ocp.compute_problem_guess_batch(S_, xg))
    _same(al_testing_batch(spec, X, fng), g["results_guess"], tol=1e-7)
    # set_bounds: the position box narrowed by 0.2 on each side; the class's spec now carries it, the oracle solves on
    # that spec, and the out-of-bounds limits (thetamin / thetamax) stay the class's, as in the reference
    before = ocp.compute_problem_batch(S)["label"]
    lo, hi = spec.thetamin + 0.2, spec.thetamax - 0.2
    ocp.set_bounds(lo, hi) if nq == 1 else ocp.set_bounds([lo] * 2, [hi] * 2)
    assert spec.xmin[0] == spec.xmin_e[nq - 1] == lo and spec.xmax[nq - 1] == spec.xmax_e[0] == hi
    assert spec.thetamin == AlSpec(nq).thetamin and spec.thetamax == AlSpec(nq).thetamax
    r2, g2 = oc.al_solve_batch(spec, S), ocp.compute_problem_batch(S)
    part = np.flatnonzero(g2["label"] != r2["label"])
    assert all(max(g2["qp_iter"][i], r2["qp_iter"][i]) >= spec.qp_iter_max for i in part) and len(part) <= 0.01 * len(S), part
    assert (r2["label"] != before).any()                     # the narrower box changes labels


class _StoredGuess:
    """A torch module whose output is a stored guess trajectory (stages 1..N), whatever the input."""

    def __init__(self, xg):
        import torch
        self.out = torch.tensor(xg[1:].reshape(1, -1), dtype=torch.float32)
        self._p = torch.nn.Parameter(torch.zeros(1))

    def parameters(self):
        return iter([self._p])

    def __call__(self, inp):
        return self.out.clone()


@pytest.mark.gpu
def test_gpu_al_chain_rules():
    """vboc_al_solve_batch's per-chain rules: nq 1, 2, 3 accepted (an empty batch is a no-op on an nq 2 handle), nq 4
    refused (VBOC_ERR_UNSUPPORTED), a spec of another chain than the handle's is a VbocError naming both."""
    import torch
    from vboc_amd import lib
    s2 = lib.Solver(2, 100)
    out = s2.al_solve_device(AlSpec(2), torch.zeros((0, 4), dtype=torch.float64, device="cuda:0"))
    torch.cuda.synchronize()
    assert out["label"].numel() == 0
    with pytest.raises(lib.VbocError, match=r"spec nq = 3 .*handle nq = 2"):
        s2.al_solve_device(AlSpec(), torch.zeros((4, 6), dtype=torch.float64, device="cuda:0"))
    s4 = lib.Solver(4, 100)
    sp4 = AlSpec(2)
    sp4.nq = 4                                             # no AlSpec exists for the arm: reach the C check
    sp4.xmin = sp4.xmin_e = np.r_[np.full(4, 2.0), np.full(4, -10.0)]
    sp4.xmax = sp4.xmax_e = np.r_[np.full(4, 4.0), np.full(4, 10.0)]
    sp4.umin, sp4.umax = np.full(4, -10.0), np.full(4, 10.0)
    sp4.W, sp4.W_e = np.zeros(12), np.zeros(8)
    with pytest.raises(lib.VbocError, match="nq = 1, 2, 3"):
        s4.al_solve_device(sp4, torch.zeros((4, 8), dtype=torch.float64, device="cuda:0"))
