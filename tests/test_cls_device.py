"""The classifier library (vboc_amd/csrc/cls.hip via learn.HipClsTrainer / ClsTrainer): the BCE fit against a plain
PyTorch restatement of the reference's loop (HJR/triplependulum_hjr.py:95-118), graph replay against eager launches,
the padding, the classification kernel and the RMSE march (:150-176) against float64 restatements.

A row (a ray) is *decided* when the float64 margin |logit1 - logit0| (at every step of the ray, up to the later of
the two stopping steps) exceeds tau = (2nq + 2 hidden + 3) 2^-24 (a3[0] + a3[1]), a3 = |W2|(|W1|(|W0||x| + |b0|) +
|b1|) + |b2|: the first-order worst case of any float32 summation order (ReLU is 1-Lipschitz).  Labels of decided
rows and step counts of decided rays must be exact; at most 5 % may be undecided (a condition on the inputs).
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
Q_MIN, Q_MAX, V_MAX = 3 * np.pi / 4, 5 * np.pi / 4, 10.0


def test_cls_library_exports_every_declared_symbol():
    import re
    from vboc_amd import clslib
    hdr = open(os.path.join(HERE, "..", "include", "vboc_cls.h")).read()
    declared = set(re.findall(r"\b(vboc_cls_\w+)\s*\(", hdr))
    assert declared == set(clslib.EXPORTS)
    lib = ctypes.CDLL(clslib.LIB_PATH)
    for name in declared:
        getattr(lib, name)
    assert clslib.supported(6, 100, 4096) and clslib.supported(4, 100, 4096) and clslib.supported(2, 100, 64)
    assert not clslib.supported(6, 500, 4096) and not clslib.supported(6, 100, 8192)


def test_make_cls_trainer_keeps_torch_on_the_cpu():
    from vboc_amd.learn import ClsTrainer, make_cls_trainer
    assert type(make_cls_trainer(3, "cpu")) is ClsTrainer
    assert type(make_cls_trainer(3, "cpu", native=True)) is ClsTrainer


def _rows(n, nq, seed=0, speed=None):
    """(F [n, 2nq + 2] float32, mean, std): candidates of the widened box, normalised as the reference does, labelled
    [0, 1] inside the state box (and, with `speed`, |v| < speed), else [1, 0]."""
    rng = np.random.default_rng(seed)
    dq, dv = (Q_MAX - Q_MIN) / 10, 2 * V_MAX / 10
    X = np.c_[rng.uniform(Q_MIN - dq, Q_MAX + dq, (n, nq)), rng.uniform(-V_MAX - dv, V_MAX + dv, (n, nq))]
    Xf = torch.from_numpy(X.astype(np.float32))
    mean, std = torch.mean(Xf), torch.std(Xf)
    inside = np.all((X[:, :nq] >= Q_MIN) & (X[:, :nq] <= Q_MAX), axis=1) & np.all(np.abs(X[:, nq:]) <= V_MAX, axis=1)
    if speed is not None:
        inside &= np.linalg.norm(X[:, nq:], axis=1) < speed
    y = torch.from_numpy(np.c_[~inside, inside].astype(np.float32))
    return torch.cat([(Xf - mean) / std, y], dim=1), mean, std


def _torch_steps(model, opt, F, nin, idx_steps, val, beta):
    crit = torch.nn.BCEWithLogitsLoss()
    for idx in idx_steps:
        ii = torch.as_tensor(idx, dtype=torch.long, device="cuda")
        loss = crit(model(F[ii, :nin]), F[ii, nin:nin + 2])
        loss.backward()
        opt.step()
        opt.zero_grad()
        val = beta * val + (1 - beta) * loss.item()
    return val


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [3, 2, 1])
def test_device_cls_fit_matches_torch_adam_bce_loop(nq):
    """The bars of test_fit_device.test_device_fit_matches_torch_adam_loop (measured for fit.hip on this hardware)."""
    import copy
    from vboc_amd.learn import HipClsTrainer
    n, nin = (30000 if nq > 1 else 3000), 2 * nq
    F = _rows(n, nq, seed=nq)[0].cuda()
    a = HipClsTrainer(nq, "cuda", seed=5)
    twin = HipClsTrainer(nq, "cuda", seed=5)
    idx = twin.sample(n, steps=5)
    ref = copy.deepcopy(a.model)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    r1 = a.fit(F, it_max=1)
    assert r1["iterations"] == 1
    v_ref = _torch_steps(ref, opt, F, nin, idx[:1], 1.0, a.beta)
    m_dev, v_dev = a.moments()
    for p, md, vd in zip(ref.parameters(), m_dev, v_dev):
        mr = opt.state[p]["exp_avg"]
        scale = float(mr.abs().max()) + 1e-30
        print("exp_avg", tuple(p.shape), float((md - mr).abs().max()) / scale)
        assert float((md - mr).abs().max()) <= 2e-5 * scale, (p.shape, float((md - mr).abs().max()), scale)
        vr = opt.state[p]["exp_avg_sq"]
        print("exp_avg_sq", tuple(p.shape), float((vd - vr).abs().max()) / (float(vr.abs().max()) + 1e-30))
        assert float((vd - vr).abs().max()) <= 5e-5 * float(vr.abs().max()) + 1e-30
    print("val", r1["val"], v_ref)
    assert abs(r1["val"] - v_ref) <= 1e-5 * abs(v_ref)
    for p, q in zip(a.model.parameters(), ref.parameters()):
        print("param 1", tuple(p.shape), float((p - q).detach().abs().max()))
        assert float((p - q).detach().abs().max()) <= 1e-5
    r2 = a.fit(F, it_max=4)
    assert r2["iterations"] == 4
    v_ref = _torch_steps(ref, opt, F, nin, idx[1:5], 1.0, a.beta)
    print("val", r2["val"], v_ref)
    assert abs(r2["val"] - v_ref) <= 1e-5 * abs(v_ref)
    for p, q in zip(a.model.parameters(), ref.parameters()):
        print("param 5", tuple(p.shape), float((p - q).detach().abs().max()))
        assert float((p - q).detach().abs().max()) <= 2e-5


@pytest.mark.gpu
def test_device_cls_graph_replay_equals_eager_and_stops_exactly():
    """poll-64 graph replays == step-by-step launches, bit for bit, on a run that stops on val (not it_max): every
    label is in one class, so the loss decays fast."""
    from vboc_amd.learn import HipClsTrainer
    F = _rows(20000, 3, seed=3)[0]
    F[:, 6], F[:, 7] = 1.0, 0.0
    a = HipClsTrainer(3, "cuda", seed=9, graphs=True, poll=64)
    b = HipClsTrainer(3, "cuda", seed=9, graphs=False, poll=1)
    ra, rb = a.fit(F, it_max=5000), b.fit(F, it_max=5000)
    assert ra["iterations"] == rb["iterations"] < 5000, (ra, rb)
    assert ra["val"] == rb["val"] and ra["val"] <= 5e-3
    assert rb["launched"] == rb["iterations"] + 1 and ra["launched"] % 64 == 0
    for p, q in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(p, q)


@pytest.mark.gpu
def test_device_cls_zero_hidden_units_stay_exactly_zero():
    """A hidden-128 twin whose units 100..127 are zero, as the padding of a hidden-100 model is: after 50 steps the
    parameters and both Adam moments of those units are still exactly zero."""
    from vboc_amd.learn import HipClsTrainer
    a = HipClsTrainer(3, "cuda", seed=2, hidden=128, stop_val=0.0)
    st = a.model.linear_relu_stack
    with torch.no_grad():
        st[0].weight[100:] = 0
        st[0].bias[100:] = 0
        st[2].weight[100:] = 0
        st[2].weight[:, 100:] = 0
        st[2].bias[100:] = 0
        st[4].weight[:, 100:] = 0
    assert a.fit(_rows(20000, 3, seed=4)[0], it_max=50)["iterations"] == 50
    for ts in [list(a.model.parameters())] + a.moments():
        W0, b0, W1, b1, W2, b2 = ts
        for t in (W0[100:], b0[100:], W1[100:], W1[:, 100:], b1[100:], W2[:, 100:]):
            assert float(t.detach().abs().max()) == 0.0
        assert float(W1[:100, :100].detach().abs().max()) > 0.0


# -- float64 restatement of the forward pass and the decided rule -----------------------------------
def _params64(model):
    return [p.detach().cpu().numpy().astype(np.float64) for p in model.parameters()]

def _forward64(W, x):
    """(logit1 - logit0, tau) per float32 row x, in float64."""
    x = x.astype(np.float64)
    h1 = np.maximum(x @ W[0].T + W[1], 0.0)
    h2 = np.maximum(h1 @ W[2].T + W[3], 0.0)
    lg = h2 @ W[4].T + W[5]
    a3 = ((np.abs(x) @ np.abs(W[0]).T + np.abs(W[1])) @ np.abs(W[2]).T + np.abs(W[3])) @ np.abs(W[4]).T + np.abs(W[5])
    tau = (W[0].shape[1] + 2 * W[0].shape[0] + 3) * 2.0 ** -24 * (a3[:, 0] + a3[:, 1])
    return lg[:, 1] - lg[:, 0], tau


def _norm32(P, mean, std):
    """(float32(P) - mean) / std in float32, as torch does with its 0-dim float32 mean / std."""
    m, s = np.float32(mean), np.float32(std)
    return (P.astype(np.float32) - m) / s


@functools.lru_cache(maxsize=None)
def _trained(nq, device):
    """A classifier with a boundary inside the velocity box: 400 steps on "inside the box and |v| < 6"."""
    from vboc_amd.learn import ClsTrainer, HipClsTrainer
    F, mean, std = _rows(30000, nq, seed=10 + nq, speed=6.0)
    tr = HipClsTrainer(nq, "cuda", seed=1, stop_val=0.0) if device == "cuda" else \
        ClsTrainer(nq, "cpu", seed=1, stop_val=0.0)
    tr.fit(F, it_max=400)
    return tr, float(mean), float(std)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 257, 70001])
def test_device_cls_eval_matches_float64_forward(n):
    tr, mean, std = _trained(3, "cuda")
    rng = np.random.default_rng(n)
    X = np.c_[rng.uniform(Q_MIN, Q_MAX, (n, 3)), rng.uniform(-12, 12, (n, 3))]
    Xn = torch.from_numpy(_norm32(X, mean, std).reshape(n, 6)).cuda()
    lab, cnt, lg = tr.predict_labels(Xn, logits=True)
    lab2, cnt2, lg2 = tr.predict_labels(Xn, logits=True)
    assert cnt == cnt2 == int(lab.sum()) and torch.equal(lab, lab2) and torch.equal(lg, lg2)
    if n == 0:
        assert cnt == 0
        return
    d, tau = _forward64(_params64(tr.model), Xn.cpu().numpy())
    decided = np.abs(d) > tau
    assert (~decided).mean() <= 0.05
    assert np.array_equal(lab.cpu().numpy()[decided], (d > 0)[decided].astype(np.uint8))
    assert np.array_equal(lab.cpu().numpy(), (lg[:, 1] > lg[:, 0]).cpu().numpy().astype(np.uint8))
    assert float((lg[:, 1] - lg[:, 0]).cpu().double().sub(torch.from_numpy(d)).abs().max()) <= float(tau.max())


def _decided(W, X, flags, T, mean, std):
    """Per ray: every point 0..T[i] of the float64 march (the reference's sequential accumulation: cumsum adds in
    order) has a float64 margin above tau."""
    nq = X.shape[1] // 2
    vt = X[:, nq:]
    c = np.where((flags & 1)[:, None] == 1, -1.0, 1.0) * ((1e-2 * vt) / np.linalg.norm(vt, axis=1)[:, None])
    out = np.zeros(X.shape[0], dtype=bool)
    for i in range(X.shape[0]):
        v = np.cumsum(np.vstack([vt[i][None], np.repeat(-c[i][None], T[i], axis=0)]), axis=0)
        d, tau = _forward64(W, _norm32(np.c_[np.repeat(X[i, :nq][None], T[i] + 1, axis=0), v], mean, std))
        out[i] = bool(np.all(np.abs(d) > tau))
    return out


def _rays(nq, W, mean, std, m=256, seed=0):
    """The rays of the march tests, all chosen by a condition on the inputs alone (the float64 margins along the
    float64 march; with steps of 1e-2 about a quarter of all random rays pass within tau of the boundary, so rays
    are drawn until enough are decided rather than seeds until a whole set is):
      * m random rays with speeds spread over [1, 10];
      * hand-made ones: start speeds one step apart below the boundary crossing of label-0 rays at speed 10 along
        eight directions (stops after 0, 1, ... 70 steps: every chunk edge of the kernel);
      * the longest: of the rays from the velocity box's corners at positions outside the state box, the one the
        classifier holds at label 0 for the most steps."""
    import itertools
    from vboc_amd.learn import march_reference
    rng = np.random.default_rng(seed)
    cls = lambda P: _forward64(W, _norm32(P, mean, std))[0] > 0

    def keep(X):
        _, steps, flags = march_reference(cls, X, mean, std)
        return _decided(W, X, flags, steps, mean, std)

    d = rng.normal(size=(4 * m, nq))
    d /= np.linalg.norm(d, axis=1)[:, None]
    X = np.c_[rng.uniform(Q_MIN, Q_MAX, (4 * m, nq)), d * np.tile(np.linspace(1.0, 10.0, m), 4)[:, None]]
    X = X[keep(X)][:m]
    assert X.shape[0] == m
    q = np.full(nq, np.pi)
    E = rng.normal(size=(8, nq))
    E /= np.linalg.norm(E, axis=1)[:, None]
    _, s0, f0 = march_reference(cls, np.c_[np.tile(q, (8, 1)), 10.0 * E], mean, std)
    assert not f0.any() and s0.min() > 100 and s0.max() < 900, (s0, f0)   # label 0 at speed 10, crossing in the box
    hand = np.array([np.r_[q, (10.0 - (s0[j] - k) * 1e-2) * E[j]] for j in range(8) for k in range(0, 71)])
    hand = hand[keep(hand)]
    far = np.array([np.r_[np.full(nq, qq), 0.99 * V_MAX * np.array(sg)]
                    for off in (0.09, 0.5, 2.0) for qq in (Q_MAX + off * (Q_MAX - Q_MIN), Q_MIN - off * (Q_MAX - Q_MIN))
                    for sg in itertools.product((-1.0, 1.0), repeat=nq)])
    far = far[keep(far)]
    far = far[np.argmax(march_reference(cls, far, mean, std)[1])]
    return np.vstack([X, hand, far[None]]), cls


def _check_march(nq, tr, mean, std, out, out128):
    from vboc_amd.learn import march_reference
    W = _params64(tr.model)
    X, cls = _rays(nq, W, mean, std)
    err, steps, flags = march_reference(cls, X, mean, std)
    m = 256
    assert (flags[:m] & 1).mean() >= 0.25 and 1 - (flags[:m] & 1).mean() >= 0.25       # both directions
    assert {1, 15, 16, 17, 63, 64, 65} <= set(steps[m:].tolist())
    assert steps[-1] > (1600 if nq == 3 else 1000) and not np.any(flags >> 1)
    g = out(X)
    # decided rays: every point up to the later stopping step has a float64 margin above tau
    decided = _decided(W, X, flags, np.maximum(steps, g["steps"]), mean, std)
    assert (~decided).mean() <= 0.05, (~decided).sum()
    assert np.array_equal(g["steps"][decided], steps[decided])
    assert np.array_equal(g["flags"][decided], flags[decided])
    assert np.abs(g["err"][decided] - err[decided]).max() <= 1e-12
    # the bound of the outward march: max_steps = 128 stops every longer ray and flags it
    g2 = out128(X)
    long = decided & (steps > 128)
    assert long.sum() > 10
    assert np.all(g2["steps"][long] == 128) and np.all((g2["flags"][long] >> 1) == 1)
    short = decided & (steps < 128)
    assert np.array_equal(g2["steps"][short], steps[short]) and not np.any(g2["flags"][short] >> 1)


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [3, 2])
def test_device_cls_march_matches_float64_restatement(nq):
    tr, mean, std = _trained(nq, "cuda")
    _check_march(nq, tr, mean, std, lambda X: tr.boundary_errors(X, mean, std),
                 lambda X: tr.boundary_errors(X, mean, std, max_steps=128))


def test_march_restatement_equals_the_reference_loop_on_8_rays():
    """learn.march_reference against a literal transcription of HJR/triplependulum_hjr.py:152-174 (one ray at a
    time, one point per classifier call), both on the float64 forward pass of a CPU-trained classifier; and the
    PyTorch path of ClsTrainer.boundary_errors (float32) against it on the decided rays."""
    from numpy.linalg import norm
    from vboc_amd.learn import march_reference
    nq = 3
    tr, mean, std = _trained(nq, "cpu")
    W = _params64(tr.model)
    X_all, cls = _rays(nq, W, mean, std)
    X_test = X_all[[3, 60, 120, 200, 255, 256 + 1, 256 + 40, len(X_all) - 1]]
    model = lambda row: int(cls(np.array([row]))[0])
    output_hjr_test = [model(X_test[i]) for i in range(len(X_test))]
    norm_error, count = np.empty((len(X_test),)), np.zeros(len(X_test), dtype=int)
    for i in range(len(X_test)):
        vel_norm = norm([X_test[i][3], X_test[i][4], X_test[i][5]])
        v0, v1, v2 = X_test[i][3], X_test[i][4], X_test[i][5]
        if output_hjr_test[i] == 0:
            out = 0
            while out == 0 and norm([v0, v1, v2]) > 1e-2:
                v0 = v0 - 1e-2 * X_test[i][3] / vel_norm
                v1 = v1 - 1e-2 * X_test[i][4] / vel_norm
                v2 = v2 - 1e-2 * X_test[i][5] / vel_norm
                out = model([X_test[i][0], X_test[i][1], X_test[i][2], v0, v1, v2])
                count[i] += 1
        else:
            out = 1
            while out == 1 and norm([v0, v1, v2]) > 1e-2:
                v0 = v0 + 1e-2 * X_test[i][3] / vel_norm
                v1 = v1 + 1e-2 * X_test[i][4] / vel_norm
                v2 = v2 + 1e-2 * X_test[i][5] / vel_norm
                out = model([X_test[i][0], X_test[i][1], X_test[i][2], v0, v1, v2])
                count[i] += 1
        norm_error[i] = vel_norm - norm([v0, v1, v2])
    err, steps, flags = march_reference(cls, X_test, mean, std)
    assert np.array_equal(steps, count) and np.array_equal(flags & 1, output_hjr_test)
    assert np.abs(err - norm_error).max() <= 1e-12
    assert count.max() > 1600
    # the CPU path of the trainer on all rays, the same checks as the device kernel's
    _check_march(nq, tr, mean, std, lambda X: tr.boundary_errors(X, mean, std),
                 lambda X: tr.boundary_errors(X, mean, std, max_steps=128))
