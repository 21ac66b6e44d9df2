"""The RMSE march on the device at the classifier's own width (vboc_pool_boundary in vboc_amd/csrc/pool.hip, through
learn.PoolScorer.boundary and pipeline.al_run(device_march=...)).

The contract that needs no tolerance: a point's label is exactly what vboc_pool_entropy writes to `labels` for a float64
row holding that point's float32 values, on the same handle.  So learn.march_reference, given that call as its
classifier, must give the kernel's `steps` and `flags` exactly, and `err` to 1e-12 (double sqrt on the device against
NumPy's: test_cls_device's bar for the same quantity).

Against float64 a ray is *decided* when every point 0..T of its float64 march (T the later of the two stopping steps)
has |logit1 - logit0| > tau_0 + tau_1, tau_o = (nin + 2 HP + 3) 2^-24 a3_o with HP the padded hidden width
(test_pool_device's bound per logit).  Step counts of decided rays must be exact.  The rays of that test are drawn
until 256 are decided along their float64 march, a condition on the inputs alone; with the device's own stopping step
included at most 5 % may then be undecided (a device that keeps the bound stops where float64 does, so none is).
"""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
Q_MIN, Q_MAX = 3 * np.pi / 4, 5 * np.pi / 4
U = 2.0 ** -24
SHAPES = [(6, 500), (4, 300), (6, 33), (4, 100)]          # NT 8, 5, 1, 2 and both NIN


# ----------------------------------------------------------------------------------------------------------------
# CPU: exports and binding, PoolScorer(native=False).boundary, al_run(device_march=...)
# ----------------------------------------------------------------------------------------------------------------
def test_pool_boundary_is_declared_bound_and_exported():
    from vboc_amd import poollib
    hdr = open(os.path.join(HERE, "..", "include", "vboc_pool.h")).read()
    assert "vboc_pool_boundary" in set(re.findall(r"\b(vboc_pool_\w+)\s*\(", hdr))
    assert "vboc_pool_boundary" in poollib.EXPORTS
    lib = ctypes.CDLL(poollib.LIB_PATH)
    assert lib.vboc_pool_boundary is not None


@functools.lru_cache(maxsize=None)
def _small_cls(nq):
    """test_al_loop's small classifier (hidden 16, 800 steps on "|v| < 9"), here for both systems and in float32."""
    from vboc_amd.learn import ClsTrainer
    rng = np.random.default_rng(1)
    Xf = np.c_[rng.uniform(Q_MIN, Q_MAX, (20000, nq)), rng.uniform(-11, 11, (20000, nq))].astype(np.float32)
    Xt = torch.from_numpy(Xf)
    mean_t, std_t = torch.mean(Xt), torch.std(Xt)
    inside = np.linalg.norm(Xf[:, nq:], axis=1) < 9.0
    F = torch.cat([(Xt - mean_t) / std_t, torch.from_numpy(np.c_[~inside, inside].astype(np.float32))], dim=1)
    tr = ClsTrainer(nq, "cpu", hidden=16, minibatch=256, lr=1e-2, stop_val=0.0, seed=3, native_eval=False)
    tr.fit(F, it_max=800)
    return tr.model, float(mean_t), float(std_t)


def _eight_rays(nq):
    """test_al_loop's 8-ray set: six ordinary rays and two whose first two velocity components are <= 1e-2 (for nq 2
    the second of them is the whole remaining velocity, so only the first component is small)."""
    rng = np.random.default_rng(1)
    d = rng.normal(size=(6, nq))
    d /= np.linalg.norm(d, axis=1)[:, None]
    special = [[0.004, -0.003, 2.0], [0.0, 0.006, -1.5]] if nq == 3 else [[0.004, 2.0], [0.006, -1.5]]
    return np.c_[rng.uniform(Q_MIN, Q_MAX, (8, nq)),
                 np.vstack([d * np.array([1.0, 2.5, 4.0, 10.5, 11.0, 12.0])[:, None], special])]


@pytest.mark.parametrize("nq,od", [(3, 2), (3, None), (2, None)])
def test_torch_path_boundary_equals_march_reference(nq, od):
    from vboc_amd.learn import PoolScorer, march_reference
    model, mean, std = _small_cls(nq)
    X = _eight_rays(nq)
    mean_t, std_t = torch.tensor(mean), torch.tensor(std)

    @torch.no_grad()
    def classify(P):
        out = model((torch.from_numpy(P) - mean_t) / std_t)
        return (out[:, 1] > out[:, 0]).numpy()

    start = classify(X.astype(np.float32))
    assert start[6] == 1 and start[7] == 1 and 0 < start[:6].sum() < 6, start
    max_steps = 3000
    err, steps, flags = march_reference(classify, X, mean, std, max_steps, od)
    sc = PoolScorer(nq, model, None, "cpu", native=False)
    b = sc.boundary(X, mean, std, max_steps=max_steps, outward_dims=od)
    assert set(b) == {"err", "steps", "flags", "capped", "rmse"}
    assert np.array_equal(b["steps"], steps) and np.array_equal(b["flags"], flags)
    assert np.abs(b["err"] - err).max() <= 1e-12
    assert b["capped"] == int(((flags >> 1) & 1).sum())
    assert b["rmse"] == math.sqrt(np.sum(np.power(b["err"], 2)) / len(X))
    assert steps[:6].min() > 0
    if od == 2:
        assert steps[6] == 0 and steps[7] == 0 and b["err"][6] == 0.0
    else:
        assert steps[6] > 100 and steps[7] > 100
    assert len(sc.calls["boundary"]) == 1
    # a device tensor or an array: to_pool takes either; the default bound is the trainer's
    b2 = sc.boundary(torch.from_numpy(X), mean, std, outward_dims=od)
    assert np.array_equal(b2["steps"], march_reference(classify, X, mean, std, outward_dims=od)[1])


@pytest.mark.parametrize("nq", [3, 2])
def test_al_run_device_march_switch_on_the_cpu(nq):
    """al_run with the stub OCP and its own PoolScorer(native=False): None and False are today's path, bit for bit;
    True raises when the scorer cannot march on the device."""
    from test_al_loop import StubOcp, StubScorer, _heldout
    from vboc_amd.al import AlSpec
    from vboc_amd.learn import PoolScorer
    from vboc_amd.pipeline import al_run
    rng = np.random.default_rng(0)
    s = AlSpec(nq)
    pool = np.c_[rng.uniform(s.thetamin, s.thetamax, (100, nq)), rng.uniform(-9, 9, (100, nq))]
    X_test = _heldout(nq, m=6, seed=3)
    a = dict(pool=pool, ocp=StubOcp(nq), B=32, N_init=32, hidden=4, minibatch=8, it_max=2, device="cpu", seed=1,
             max_iterations=1)
    r0 = al_run(nq, X_test, device_march=None, **a)
    r1 = al_run(nq, X_test, device_march=False, **a)
    assert type(r0["scorer"]) is PoolScorer and not r0["scorer"].native
    assert r0["iterations"] == 1 and len(r0["rmse"]) == 2 and np.all(np.isfinite(r0["rmse"]))
    assert np.array_equal(r0["rmse"], r1["rmse"])
    assert len(r0["capped"]) == 2 and r0["capped"] == r1["capped"] and all(isinstance(c, int) for c in r0["capped"])
    assert len(r0["march_s"]) == 2 and r0["split"]["march"] > 0
    # the march of the final model again, through the scorer's torch path: al_run's own rmse
    b = r0["scorer"].boundary(X_test, r0["mean"], r0["std"], outward_dims=2 if nq == 3 else None)
    assert b["rmse"] == r0["rmse"][-1] and b["capped"] == r0["capped"][-1]
    with pytest.raises(ValueError):
        al_run(nq, X_test, device_march=True, **a)
    stub = dict(a, scorer=StubScorer(nq, [0.5]))
    with pytest.raises(ValueError):
        al_run(nq, X_test, device_march=True, **stub)
    r2 = al_run(nq, X_test, **stub)                     # a scorer without `boundary` keeps working
    assert len(r2["capped"]) == 2 and len(r2["rmse"]) == 2
    assert al_run(nq, None, **stub)["capped"] == [0, 0]


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _lib_labels(sc, P, mean, std):
    """vboc_pool_entropy's `labels` of P.astype(float64) on the scorer's handle."""
    X = torch.from_numpy(np.ascontiguousarray(P, dtype=np.float64)).cuda()
    n = X.shape[0]
    etp = torch.empty((n,), dtype=torch.float32, device="cuda")
    lab = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    if n:
        sc._pl.check(sc._lib.vboc_pool_entropy(sc._h, X.data_ptr(), n, float(mean), float(std), etp.data_ptr(), None,
                                               lab.data_ptr(), sc._stream()))
    lab = lab.cpu().numpy()
    assert np.all(lab <= 1)
    return lab


SENT = (-7.0, -7, 77)       # what the outputs hold before a call


def _lib_march(sc, X, mean, std, max_steps, od, m=None, h=None):
    """One vboc_pool_boundary call: (rc, err, steps, flags); the outputs are filled with SENT before it."""
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).cuda()
    n = Xd.shape[0]
    err = torch.full((max(n, 1),), SENT[0], dtype=torch.float64, device="cuda")
    steps = torch.full((max(n, 1),), SENT[1], dtype=torch.int32, device="cuda")
    flags = torch.full((max(n, 1),), SENT[2], dtype=torch.uint8, device="cuda")
    rc = sc._lib.vboc_pool_boundary(sc._h if h is None else h, Xd.data_ptr() if n else None, n if m is None else m,
                                    float(mean), float(std), max_steps, od, err.data_ptr(), steps.data_ptr(),
                                    flags.data_ptr(), sc._stream())
    torch.cuda.synchronize()
    return rc, err.cpu().numpy()[:n], steps.cpu().numpy()[:n], flags.cpu().numpy()[:n]


def _push(sc):
    sc._pl.check(sc._lib.vboc_pool_set_classifier(sc._h, *sc._ptrs(sc.cls_model), sc._stream()))


def _scorer(model):
    from vboc_amd.learn import PoolScorer
    model = model.cuda()
    sc = PoolScorer(model.linear_relu_stack[0].in_features // 2, model, None, "cuda")
    _push(sc)
    return sc


@functools.lru_cache(maxsize=None)
def _ball_cls(nin, hidden):
    """(module on the CPU, mean, std): a ClsTrainer after 80 torch steps on the ball labels "|v| < 6" over velocities
    in [-8, 8] (as test_cls_device._trained does, without the state box: the ball then is a fifth to a half of the
    rows, and 80 steps find it), trained on the CPU so that the weights do not depend on the card."""
    from vboc_amd.learn import ClsTrainer
    nq = nin // 2
    rng = np.random.default_rng(10 + nq)
    X = np.c_[rng.uniform(Q_MIN, Q_MAX, (30000, nq)), rng.uniform(-8.0, 8.0, (30000, nq))]
    Xf = torch.from_numpy(X.astype(np.float32))
    mean, std = torch.mean(Xf), torch.std(Xf)
    inside = np.linalg.norm(X[:, nq:], axis=1) < 6.0
    F = torch.cat([(Xf - mean) / std, torch.from_numpy(np.c_[~inside, inside].astype(np.float32))], dim=1)
    tr = ClsTrainer(nq, "cpu", hidden=hidden, minibatch=1024, lr=1e-2, stop_val=0.0, seed=1, native_eval=False)
    tr.fit(F, it_max=80)
    return tr.model, float(mean), float(std)


def _rays(nq, m, seed, lo=1.0, hi=10.0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(m, nq))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.c_[rng.uniform(Q_MIN, Q_MAX, (m, nq)), d * rng.uniform(lo, hi, (m, 1))]


G1_STEPS = 300      # the bound of G1's marches: the float32 classifier of 60 steps may hold an outward ray for long


@functools.lru_cache(maxsize=None)
def _g1(nin, hidden, od):
    """Shared by G1 and G4: (scorer, X [257], mean, std, march_reference under the library's labels).  The triple's
    last four rays have first two velocity components <= 1e-2: outward_dims = 2 takes no step on them when they
    start at label 1."""
    from vboc_amd.learn import march_reference
    model, mean, std = _ball_cls(nin, hidden)
    sc = _scorer(model)
    X = _rays(nin // 2, 257, seed=nin + hidden)
    if nin == 6:
        X[-4:, 3:] = [[0.004, -0.003, 2.0], [0.0, 0.006, -1.5], [0.003, 0.002, 4.0], [-0.005, 0.001, -3.0]]
    ref = march_reference(lambda P: _lib_labels(sc, P, mean, std), X, mean, std, G1_STEPS, od or None)
    return sc, X, mean, std, ref


@pytest.mark.gpu
@pytest.mark.parametrize("nin,hidden,od", [(n, h, od) for n, h in SHAPES for od in ((0, 2) if n == 6 else (0,))])
def test_march_equals_march_reference_under_the_librarys_own_labels(nin, hidden, od):
    """G1: exact, with no carve-out."""
    from vboc_amd.learn import march_reference
    sc, X, mean, std, (err, steps, flags) = _g1(nin, hidden, od)
    lab = flags & 1
    print("label 1:", lab.mean(), "steps min / max:", steps.min(), steps.max(), "capped:", (flags >> 1).sum())
    assert 0.1 <= lab.mean() <= 0.9                      # conditions on the inputs
    assert np.any((steps > 0) & (steps <= 63)) and np.any(steps >= 129)
    if od == 2:
        assert np.any((steps[-4:] == 0) & (lab[-4:] == 1))
    rc, e, s, f = _lib_march(sc, X, mean, std, G1_STEPS, od)
    assert rc == 0
    assert np.array_equal(s, steps) and np.array_equal(f, flags)
    print("err difference:", np.abs(e - err).max())
    assert np.abs(e - err).max() <= 1e-12
    # m = 1 and m = 0
    rc, e1, s1, f1 = _lib_march(sc, X[:1], mean, std, G1_STEPS, od)
    r1 = march_reference(lambda P: _lib_labels(sc, P, mean, std), X[:1], mean, std, G1_STEPS, od or None)
    assert rc == 0 and s1[0] == r1[1][0] == steps[0] and f1[0] == r1[2][0] and abs(e1[0] - r1[0][0]) <= 1e-12
    rc, e0, s0, f0 = _lib_march(sc, X[:0], mean, std, G1_STEPS, od)
    assert rc == 0 and e0.shape == (0,)
    b = sc.boundary(X[:0], mean, std, outward_dims=od)
    assert b["err"].shape == (0,) and b["steps"].shape == (0,) and b["rmse"] == 0.0 and b["capped"] == 0
    # through PoolScorer.boundary: the same call, with rmse and capped on the host
    b = sc.boundary(X, mean, std, max_steps=G1_STEPS, outward_dims=od)
    assert np.array_equal(b["steps"], s) and np.array_equal(b["flags"], f) and np.array_equal(b["err"], e)
    assert b["capped"] == int(((f >> 1) & 1).sum()) and b["rmse"] == math.sqrt(np.sum(np.power(e, 2)) / 257)


# -- G2: analytic classifiers ----------------------------------------------------------------------------------
def _l1_ball(nq, r):
    """NeuralNetCLS(2nq, 2nq, 2) with logit0 = sum |v_i| and logit1 = r (mean 0, std 1): label 1 inside the L1 ball
    of radius r.  Hidden units relu(+-v_i), the second layer the identity."""
    from vboc_amd.learn import NeuralNetCLS
    model = NeuralNetCLS(2 * nq, 2 * nq, 2)
    st = model.linear_relu_stack
    with torch.no_grad():
        for p in model.parameters():
            p.zero_()
        for i in range(nq):
            st[0].weight[i, nq + i] = 1.0
            st[0].weight[nq + i, nq + i] = -1.0
        st[2].weight.copy_(torch.eye(2 * nq))
        st[4].weight[0, :] = 1.0
        st[4].bias[1] = float(r)
    return model


def _dir(nq):
    d = np.array([0.6, -0.5, 0.62])[:nq]
    return d / np.linalg.norm(d)


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [3, 2])
def test_march_always_label_0_ends_on_the_norm_across_round_edges(nq):
    """The sequential accumulation and the hand-over between rounds of 64 points: rays that end just before, at and
    just after the first round's last point (0.66 and 0.67 are there so that 63, 64 and 65 steps all occur whichever
    way the accumulated roundings fall), in the third and in the fifth round, and one that takes no step."""
    from vboc_amd.learn import march_reference
    sc = _scorer(_l1_ball(nq, -1.0))
    q = np.full(nq, np.pi)
    X = np.array([np.r_[q, s * _dir(nq)] for s in (0.005, 0.63, 0.64, 0.65, 0.66, 0.67, 1.5, 3.0)])
    err, steps, flags = march_reference(lambda P: np.zeros(len(P), dtype=np.int64), X, 0.0, 1.0)
    print("steps", steps)
    assert steps[0] == 0 and {63, 64, 65} <= set(steps.tolist()) and not flags.any()
    assert (steps[6] - 1) // 64 == 2 and (steps[7] - 1) // 64 == 4
    rc, e, s, f = _lib_march(sc, X, 0.0, 1.0, 0, 0)
    assert rc == 0 and np.array_equal(s, steps) and np.array_equal(f, flags) and np.abs(e - err).max() <= 1e-12
    assert e[0] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [3, 2])
def test_march_always_label_1_ends_on_max_steps(nq):
    from vboc_amd.learn import march_reference
    sc = _scorer(_l1_ball(nq, 1e6))
    X = _rays(nq, 5, seed=nq, lo=0.5, hi=8.0)
    for max_steps in (1, 5, 63, 64, 65, 130):
        err, steps, flags = march_reference(lambda P: np.ones(len(P), dtype=np.int64), X, 0.0, 1.0, max_steps)
        assert np.all(steps == max_steps) and np.all(flags == 3)
        rc, e, s, f = _lib_march(sc, X, 0.0, 1.0, max_steps, 0)
        assert rc == 0 and np.all(s == max_steps) and np.all(f == 3), (max_steps, s, f)
        assert np.abs(e - err).max() <= 1e-12


@pytest.mark.gpu
def test_march_outward_dims_decides_whether_a_ray_steps_at_all():
    from vboc_amd.learn import march_reference
    sc = _scorer(_l1_ball(3, 1e6))
    q = np.full(3, np.pi)
    X = np.array([np.r_[q, 0.004, -0.003, 2.0], np.r_[q, 0.0, 0.006, -1.5], np.r_[q, 0.3, -0.2, 0.1]])
    ones = lambda P: np.ones(len(P), dtype=np.int64)
    rc, e, s, f = _lib_march(sc, X, 0.0, 1.0, 5, 2)
    assert rc == 0 and list(s) == [0, 0, 5] and list(f) == [1, 1, 3] and e[0] == 0.0 and e[1] == 0.0
    err, steps, flags = march_reference(ones, X, 0.0, 1.0, 5, 2)
    assert np.array_equal(s, steps) and np.array_equal(f, flags) and np.abs(e - err).max() <= 1e-12
    for od in (0, 3):
        rc, e, s, f = _lib_march(sc, X, 0.0, 1.0, 5, od)
        err, steps, flags = march_reference(ones, X, 0.0, 1.0, 5)
        assert rc == 0 and list(s) == [5, 5, 5] and list(f) == [3, 3, 3] and np.abs(e - err).max() <= 1e-12
    # outward_dims = 1: the first component alone
    rc, e, s, f = _lib_march(sc, X, 0.0, 1.0, 5, 1)
    err, steps, flags = march_reference(ones, X, 0.0, 1.0, 5, 1)
    assert rc == 0 and list(s) == [0, 0, 5] and np.array_equal(s, steps) and np.array_equal(f, flags)


# -- float64 and the decided rule ------------------------------------------------------------------------------
def _padded(hidden):
    return next(64 * nt for nt in (1, 2, 4, 5, 8) if hidden <= 64 * nt)


def _margin64(W, P, mean, std, dev):
    """(logit1 - logit0, tau_0 + tau_1) of the float32 rows P, the forward in float64 (torch, on `dev`)."""
    x = torch.from_numpy(((P.astype(np.float32) - np.float32(mean)) / np.float32(std)).astype(np.float64)).to(dev)
    h1 = torch.relu(x @ W[0].T + W[1])
    h2 = torch.relu(h1 @ W[2].T + W[3])
    lg = h2 @ W[4].T + W[5]
    a3 = ((x.abs() @ W[0].abs().T + W[1].abs()) @ W[2].abs().T + W[3].abs()) @ W[4].abs().T + W[5].abs()
    tau = (W[0].shape[1] + 2 * _padded(W[0].shape[0]) + 3) * U * (a3[:, 0] + a3[:, 1])
    return (lg[:, 1] - lg[:, 0]).cpu().numpy(), tau.cpu().numpy()


def _w64(model, dev):
    return [p.detach().to(dev, torch.float64) for p in model.parameters()]


def _decided(W, X, label, T, mean, std, dev):
    """Per ray: every point 0..T[i] of the float64 march (sequential accumulation: cumsum adds in order) has a
    float64 margin above tau.  One batched forward over all the points."""
    nq = X.shape[1] // 2
    vt = X[:, nq:]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(label[:, None] == 1, -1.0, 1.0) * ((1e-2 * vt) / np.linalg.norm(vt, axis=1)[:, None])
    pts, owner = [], []
    for i in range(X.shape[0]):
        v = np.cumsum(np.vstack([vt[i][None], np.repeat(-c[i][None], T[i], axis=0)]), axis=0)
        pts.append(np.c_[np.repeat(X[i, :nq][None], T[i] + 1, axis=0), v])
        owner.append(np.full(T[i] + 1, i))
    d, tau = _margin64(W, np.vstack(pts), mean, std, dev)
    bad = np.zeros(X.shape[0], dtype=np.int64)
    np.add.at(bad, np.concatenate(owner), ~(np.abs(d) > tau))
    return bad == 0


def check_against_float64(model, mean, std, nq, od, march, dev, max_steps=192, want=256):
    """G3.  Rays are drawn until `want` are decided along their float64 march (a condition on the inputs alone);
    then, with the device's own stopping step included, at most 5 % are undecided, and on the decided rays steps and
    flags are exact and err agrees to 1e-12.  Speeds in [3, 9] around the ball of radius 6 and the bound max_steps
    keep the marches short."""
    from vboc_amd.learn import march_reference
    W = _w64(model, dev)
    cls64 = lambda P: _margin64(W, P, mean, std, dev)[0] > 0
    got, drawn = [], 0
    for batch in range(16):
        Xb = _rays(nq, want, seed=100 * (batch + 1) + nq + model.linear_relu_stack[0].out_features, lo=3.0, hi=9.0)
        _, sb, fb = march_reference(cls64, Xb, mean, std, max_steps, od)
        got.append(Xb[_decided(W, Xb, fb & 1, sb, mean, std, dev)])
        drawn += want
        if sum(len(g) for g in got) >= want:
            break
    X = np.vstack(got)[:want]
    print("rays drawn:", drawn)
    assert len(X) == want, len(X)
    err, steps, flags = march_reference(cls64, X, mean, std, max_steps, od)
    assert 0.1 <= (flags & 1).mean() <= 0.9
    g = march(X, max_steps)
    assert np.array_equal(g["flags"] & 1, flags & 1)        # the start points are decided
    decided = _decided(W, X, flags & 1, np.maximum(steps, g["steps"]), mean, std, dev)
    print("undecided:", int((~decided).sum()), "of", want, "steps max:", steps.max(), "capped:", (flags >> 1).sum())
    assert (~decided).mean() <= 0.05
    assert np.array_equal(g["steps"][decided], steps[decided])
    assert np.array_equal(g["flags"][decided], flags[decided])
    assert np.abs(g["err"][decided] - err[decided]).max() <= 1e-12
    return X, decided


@pytest.mark.parametrize("od", [None, 2])
def test_float64_check_holds_for_the_torch_path_on_the_cpu(od):
    """The G3 check itself, run on the CPU against PoolScorer(native=False) at a small width."""
    from vboc_amd.learn import PoolScorer
    model, mean, std = _ball_cls(6, 33)
    sc = PoolScorer(3, model, None, "cpu", native=False)
    check_against_float64(model, mean, std, 3, od, lambda X, ms: sc.boundary(X, mean, std, ms, od), "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("nin,hidden,od", [(n, h, od) for n, h in SHAPES for od in ((None, 2) if n == 6 else (None,))])
def test_march_matches_float64_on_decided_rays(nin, hidden, od):
    """G3."""
    model, mean, std = _ball_cls(nin, hidden)
    sc = _scorer(model)
    check_against_float64(model, mean, std, nin // 2, od, lambda X, ms: sc.boundary(X, mean, std, ms, od), "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [3, 2])
def test_march_finite_l1_ball_matches_float64_on_decided_rays(nq):
    """G2, a finite ball (r = 2): inward and outward rays end where the float64 restatement's do."""
    from vboc_amd.learn import march_reference
    model = _l1_ball(nq, 2.0)
    sc = _scorer(model)
    W = _w64(model, "cuda")
    X = _rays(nq, 64, seed=7 + nq, lo=0.2, hi=4.0)
    err, steps, flags = march_reference(lambda P: _margin64(W, P, 0.0, 1.0, "cuda")[0] > 0, X, 0.0, 1.0, 512)
    assert 0.1 <= (flags & 1).mean() <= 0.9 and not np.any(flags >> 1) and steps.max() > 128
    rc, e, s, f = _lib_march(sc, X, 0.0, 1.0, 512, 0)
    assert rc == 0
    decided = _decided(W, X, flags & 1, np.maximum(steps, s), 0.0, 1.0, "cuda")
    print("undecided:", int((~decided).sum()), "of", len(X))
    assert (~decided).mean() <= 0.05
    assert np.array_equal(s[decided], steps[decided]) and np.array_equal(f[decided], flags[decided])
    assert np.abs(e[decided] - err[decided]).max() <= 1e-12


# -- G4: independence and repeatability ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nin,hidden", SHAPES)
def test_march_is_repeatable_and_a_ray_does_not_depend_on_its_batch(nin, hidden):
    od = 2 if nin == 6 else 0
    sc, X, mean, std, _ = _g1(nin, hidden, od)
    _push(sc)
    rc, e, s, f = _lib_march(sc, X, mean, std, G1_STEPS, od)
    rc2, e2, s2, f2 = _lib_march(sc, X, mean, std, G1_STEPS, od)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(e, e2) and np.array_equal(s, s2) and np.array_equal(f, f2)
    for i in (0, 63, 64, 200, 256):
        rc1, e1, s1, f1 = _lib_march(sc, X[i:i + 1], mean, std, G1_STEPS, od)
        assert rc1 == 0 and e1[0] == e[i] and s1[0] == s[i] and f1[0] == f[i]
    # an entropy pass in between leaves the march's bits alone
    _lib_labels(sc, X.astype(np.float32), mean, std)
    rc3, e3, s3, f3 = _lib_march(sc, X, mean, std, G1_STEPS, od)
    assert rc3 == 0 and np.array_equal(e, e3) and np.array_equal(s, s3) and np.array_equal(f, f3)
    # other weights on the same handle: the march follows them
    import copy
    other = copy.deepcopy(sc.cls_model)
    with torch.no_grad():
        other.linear_relu_stack[4].bias[0] = 1e6        # logit0 huge: every point is label 0
    keep, sc.cls_model = sc.cls_model, other
    try:
        _push(sc)
        rc4, e4, s4, f4 = _lib_march(sc, X, mean, std, G1_STEPS, od)
    finally:
        sc.cls_model = keep
        _push(sc)
    from vboc_amd.learn import march_reference
    err0, steps0, flags0 = march_reference(lambda P: np.zeros(len(P), dtype=np.int64), X, mean, std, G1_STEPS)
    assert rc4 == 0 and np.array_equal(s4, steps0) and np.array_equal(f4, flags0) and np.abs(e4 - err0).max() <= 1e-12
    assert not np.array_equal(s4, s)
    rc5, e5, s5, f5 = _lib_march(sc, X, mean, std, G1_STEPS, od)
    assert rc5 == 0 and np.array_equal(e, e5) and np.array_equal(s, s5) and np.array_equal(f, f5)


# -- G5: arguments ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_march_arguments():
    from vboc_amd import poollib
    from vboc_amd.learn import NeuralNetCLS, PoolScorer
    sc = _scorer(_l1_ball(3, 1e6))
    X = _rays(3, 4, seed=1)

    def untouched(r):
        return np.all(r[1] == SENT[0]) and np.all(r[2] == SENT[1]) and np.all(r[3] == SENT[2])

    for kw in (dict(max_steps=(1 << 20) + 1, od=0), dict(max_steps=5, od=0, m=-1), dict(max_steps=5, od=4),
               dict(max_steps=5, od=-1)):
        r = _lib_march(sc, X, 0.0, 1.0, **kw)
        assert r[0] == poollib.EARG and untouched(r), kw
    assert _lib_march(sc, X, 0.0, 1.0, 1 << 20, 0, m=0)[0] == 0
    # max_steps = 0 behaves as 16 384: the always-1 classifier holds every ray to the bound
    rc, e, s, f = _lib_march(sc, X, 0.0, 1.0, 0, 0)
    rc2, e2, s2, f2 = _lib_march(sc, X, 0.0, 1.0, 16384, 0)
    assert rc == 0 and rc2 == 0 and np.all(s == 16384) and np.all(f == 3)
    assert np.array_equal(e, e2) and np.array_equal(s, s2) and np.array_equal(f, f2)
    # inputs 2: no reference driver marches the pendulum
    p = PoolScorer(1, NeuralNetCLS(2, 8, 2).cuda(), None, "cuda")
    _push(p)
    r = _lib_march(p, np.array([[3.0, 1.0]]), 0.0, 1.0, 5, 0)
    assert r[0] == poollib.EUNSUPPORTED and untouched(r)
    # a handle with no classifier set fails the way vboc_pool_entropy does
    fresh = PoolScorer(3, NeuralNetCLS(6, 8, 2).cuda(), None, "cuda")
    r = _lib_march(fresh, X, 0.0, 1.0, 5, 0)
    assert r[0] == poollib.EARG and untouched(r)
    with pytest.raises(poollib.PoolError):
        sc._pl.check(r[0])


# -- G6: in the loop -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nq", [3, 2])
def test_al_run_marches_on_the_device(nq):
    """test_al_run_on_the_device_scorer's run (pool 4096, N_init = B = 256, hidden 100, two iterations, 50 rays)."""
    from test_al_loop import _heldout, _pool
    from vboc_amd.learn import PoolScorer
    from vboc_amd.pipeline import al_run
    X_test = _heldout(nq, m=50, seed=5)
    r = al_run(nq, X_test, pool=_pool(nq, 4096, seed=40 + nq), B=256, N_init=256, hidden=100, minibatch=64, it_max=20,
               max_iterations=2, seed=3, device="cuda")
    od = 2 if nq == 3 else None
    assert r["device_march"] and r["split"]["march"] > 0 and len(r["capped"]) == 3 and len(r["rmse"]) == 3
    assert len(r["scorer"].calls["boundary"]) == 3
    mean, std = r["mean"], r["std"]
    b = r["scorer"].boundary(X_test, mean, std, outward_dims=od)
    assert b["rmse"] == r["rmse"][-1] and b["capped"] == r["capped"][-1]
    # the torch path on the same module, on the rays decided by the float64 rule
    model = r["trainer"].model
    t = PoolScorer(nq, model, None, "cuda", native=False).boundary(X_test, mean, std, outward_dims=od)
    W = _w64(model, "cuda")
    decided = _decided(W, X_test, b["flags"] & 1, np.maximum(b["steps"], t["steps"]), float(mean), float(std), "cuda")
    print("decided:", int(decided.sum()), "of 50; steps", b["steps"].min(), b["steps"].max(), "capped", r["capped"])
    assert decided.any()
    assert np.array_equal(b["steps"][decided], t["steps"][decided])
    assert np.array_equal(b["flags"][decided], t["flags"][decided])
