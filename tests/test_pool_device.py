"""The pool library of the AL loop (vboc_amd/csrc/pool.hip via learn.PoolScorer): the entropy of the unlabeled pool, the
top-B selection with the pool's compaction, and the guess network's trajectories, against float64 restatements.

The forward bound is tests/test_cls_device.py::_forward64's, per output: tau = (nin + 2 H + 3) 2^-24 a3, with
a3 = |W2|(|W1|(|W0||x| + |b0|) + |b1|) + |b2| and H the padded hidden width: the first-order worst case of any float32
summation order of the three layers (nin + 1, H + 1 and H + 1 rounded operations; ReLU is 1-Lipschitz).
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
Q_MIN, Q_MAX, V_MAX = 3 * np.pi / 4, 5 * np.pi / 4, 10.0
U = 2.0 ** -24
ETP_TOL = 2.0 ** -20        # see entropy64_of_logits


def test_pool_library_exports_every_declared_symbol():
    from vboc_amd import poollib
    hdr = open(os.path.join(HERE, "..", "include", "vboc_pool.h")).read()
    declared = set(re.findall(r"\b(vboc_pool_\w+)\s*\(", hdr))
    assert declared == set(poollib.EXPORTS)
    lib = ctypes.CDLL(poollib.LIB_PATH)
    for name in declared:
        getattr(lib, name)
    assert poollib.supported(6, 500) and poollib.supported(4, 300) and poollib.supported(2, 100)
    assert poollib.supported(6, 1) and poollib.supported(6, 512, 600) and poollib.supported(4, 300, 400)
    assert poollib.supported(6, 512, 638) is False          # not a multiple of the inputs
    assert not poollib.supported(6, 513) and not poollib.supported(3, 100) and not poollib.supported(6, 500, 641)
    assert not poollib.supported(6, 0) and not poollib.supported(4, 300, 644)


# -- float64 restatements ---------------------------------------------------------------------------
def padded(hidden):
    return next(64 * nt for nt in (1, 2, 4, 5, 8) if hidden <= 64 * nt)


def norm32(P, mean, std):
    """(float32(P) - mean) / std in float32, as torch does with its 0-dim float32 mean / std."""
    return (P.astype(np.float32) - np.float32(mean)) / np.float32(std)


def forward64(W, x):
    """(outputs [n, O], a3 [n, O]) of the float32 rows x in float64; tau = (nin + 2 H + 3) 2^-24 a3 per output."""
    x = x.astype(np.float64)
    h1 = np.maximum(x @ W[0].T + W[1], 0.0)
    h2 = np.maximum(h1 @ W[2].T + W[3], 0.0)
    out = h2 @ W[4].T + W[5]
    a3 = ((np.abs(x) @ np.abs(W[0]).T + np.abs(W[1])) @ np.abs(W[2]).T + np.abs(W[3])) @ np.abs(W[4]).T + np.abs(W[5])
    return out, a3


def params64(model):
    return [p.detach().cpu().numpy().astype(np.float64) for p in model.parameters()]


def entropy64_of_logits(lg):
    """scipy.stats.entropy(sigmoid(l)) in float64.  The kernel's float32 value is within 2^-20 of it on the same
    logits: p = 1 / (1 + exp(-l)), q = p / (p0 + p1), -(q0 log q0 + q1 log q1) are under 16 rounded float32
    operations on quantities <= 1, and each term's sensitivity to its q's relative error, |q (log q + 1)|, is <= 1
    (q log q itself <= 1 / e): 16 x 2^-24."""
    lg = lg.astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-lg))
    q = p / p.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(q > 0, -q * np.log(q), 0.0)
    return t.sum(axis=1)


def entropy64(W, X, mean, std):
    """(float64 entropy of the raw rows X, eps) with eps the bound of a device score against it:
        |etp32 - H(l64)| <= |etp32 - H(l32)| + |H(l32) - H(l64)| <= 2^-20 + (tau_0 + tau_1) / 4.
    H as a function of the logits has dH/dl_o = -+ log(q1 / q0) q0 q1 (1 - p_o), and q (1 - q) |log((1 - q) / q)| has
    its maximum 0.2240 < 1 / 4 on (0, 1) (at q = 0.176), so H is 1/4-Lipschitz in each logit; tau_o is the forward
    bound of the module docstring with the padded width.  eps is the largest such bound over the rows."""
    H = padded(W[0].shape[0])
    lg, a3 = forward64(W, norm32(X, mean, std))
    tau = (W[0].shape[1] + 2 * H + 3) * U * a3
    return entropy64_of_logits(lg), float(ETP_TOL + 0.25 * (tau[:, 0] + tau[:, 1]).max())


def ranking_ok(e64, eps, idx, B):
    """The device's choice idx of the B most uncertain rows against the float64 entropies: with t64 the B-th largest
    float64 entropy, every selected row has e64 >= t64 - 2 eps and every row above t64 + 2 eps is selected (a device
    score is within eps of e64, so the device's own threshold is within eps of t64)."""
    t64 = np.sort(e64)[-B]
    sel = np.zeros(e64.shape[0], dtype=bool)
    sel[idx] = True
    assert sel.sum() == B == len(idx)
    assert np.all(e64[sel] >= t64 - 2 * eps), (float(e64[sel].min()), float(t64), eps)
    assert np.all(sel[e64 > t64 + 2 * eps])


@functools.lru_cache(maxsize=None)
def trained(nin, hidden):
    """(model on the GPU, mean, std): NeuralNetCLS(nin, hidden, 2) after 300 torch steps on "inside the box and
    |v| < 6" (as test_cls_device._trained does): the boundary, and so a spread of entropies, lies inside the pool."""
    from vboc_amd.learn import NeuralNetCLS
    nq = nin // 2
    rng = np.random.default_rng(nin)
    n = 20000
    X = np.c_[rng.uniform(Q_MIN - 0.15, Q_MAX + 0.15, (n, nq)), rng.uniform(-12, 12, (n, nq))]
    Xf = torch.from_numpy(X.astype(np.float32))
    mean, std = torch.mean(Xf), torch.std(Xf)
    inside = np.all((X[:, :nq] >= Q_MIN) & (X[:, :nq] <= Q_MAX), axis=1) & (np.linalg.norm(X[:, nq:], axis=1) < 6.0)
    y = torch.from_numpy(np.c_[~inside, inside].astype(np.float32)).cuda()
    Xn = ((Xf - mean) / std).cuda()
    torch.manual_seed(hidden)
    model = NeuralNetCLS(nin, hidden, 2).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    crit = torch.nn.BCEWithLogitsLoss()
    g = torch.Generator().manual_seed(1)
    for _ in range(300):
        ii = torch.randint(0, n, (1024,), generator=g).cuda()
        loss = crit(model(Xn[ii]), y[ii])
        loss.backward()
        opt.step()
        opt.zero_grad()
    return model, float(mean), float(std)


def pool_rows(nin, n, seed):
    nq = nin // 2
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(Q_MIN, Q_MAX, (n, nq)), rng.uniform(-11, 11, (n, nq))]


@functools.lru_cache(maxsize=None)
def scored(nin, hidden, n):
    """One shared pass: (scorer, X, X on the device, etp, logits) of the trained classifier over n pool rows."""
    from vboc_amd.learn import PoolScorer
    model, mean, std = trained(nin, hidden)
    sc = PoolScorer(nin // 2, model, None, "cuda")
    X = pool_rows(nin, n, seed=n + hidden)
    Xd = sc.to_pool(X)
    etp, lg = sc.entropy(Xd, mean, std, logits=True)
    return sc, X, Xd, etp, lg


# -- the entropy ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 257, 70001])
@pytest.mark.parametrize("nin,hidden", [(6, 500), (4, 300), (2, 100), (6, 33)])
def test_pool_entropy_matches_float64_forward(nin, hidden, n):
    model, mean, std = trained(nin, hidden)
    sc, X, Xd, etp, lg = scored(nin, hidden, n)
    assert etp.shape == (n,) and lg.shape == (n, 2) and etp.dtype == torch.float32
    if n == 0:
        return
    etp2, lg2 = sc.entropy(Xd, mean, std, logits=True)
    assert torch.equal(etp, etp2) and torch.equal(lg, lg2)
    W = params64(model)
    H = padded(hidden)
    lg64, a3 = forward64(W, norm32(X, mean, std))
    tau = (nin + 2 * H + 3) * U * a3
    lgh = lg.cpu().numpy()
    err = np.abs(lgh.astype(np.float64) - lg64)
    print("logit error / bound", float((err / tau).max()))
    assert np.all(err <= tau)
    e = etp.cpu().numpy()
    assert np.all(np.isfinite(e)) and np.all(e >= 0) and not np.any(np.signbit(e))
    d = np.abs(e.astype(np.float64) - entropy64_of_logits(lgh))
    print("entropy error", float(d.max()), "spread", float(e.min()), float(e.max()))
    assert d.max() <= ETP_TOL
    if n == 70001:
        assert e.max() > 0.6 and e.min() < 0.05             # the boundary is inside the pool
        for i in (0, 63, 64, 12345, 69951, 70000):          # a row alone scores as it does inside the batch
            e1, l1 = sc.entropy(Xd[i:i + 1].contiguous(), mean, std, logits=True)
            assert torch.equal(e1[0], etp[i]) and torch.equal(l1[0], lg[i])


# -- the selection ----------------------------------------------------------------------------------
def _scores(kind, n, rng):
    if kind == "distinct":
        s = rng.permutation(n).astype(np.float32) / np.float32(max(n, 1))
    elif kind == "ties":
        s = (rng.integers(0, 8, n) / 8.0).astype(np.float32)
    elif kind == "equal":
        s = np.full(n, 0.25, dtype=np.float32)
    else:                                                   # zeros of both signs among small scores
        s = rng.choice(np.array([0.0, -0.0, 0.0, 0.5, 0.125], dtype=np.float32), n)
        s[0] = np.float32(-0.0)
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["distinct", "ties", "equal", "zeros"])
@pytest.mark.parametrize("n", [1, 1000, 70001])
def test_pool_selection_is_exact(n, kind):
    from vboc_amd.learn import NeuralNetCLS, PoolScorer
    sc = PoolScorer(3, NeuralNetCLS(6, 8, 2).cuda(), None, "cuda")
    rng = np.random.default_rng(n + len(kind))
    s = _scores(kind, n, rng)
    X = rng.normal(size=(n, 6))
    sd, Xd = torch.from_numpy(s).cuda(), torch.from_numpy(X).cuda()
    for B in sorted({b for b in (1, 37, n // 2, n) if 1 <= b <= n}):
        want = np.sort(np.argsort(-s, kind="stable")[:B])[::-1]
        r = sc.select(sd, Xd, B)
        assert np.array_equal(r["idx"], want), (n, kind, B)
        assert np.array_equal(r["X_sel"].cpu().numpy(), X[want])
        assert np.array_equal(r["X_rest"].cpu().numpy(), np.delete(X, want, 0))
        assert r["etpmax"] == float(s[want].max()) and np.array_equal(r["scores"], s[want])
    # B > n is the caller's to clamp
    from vboc_amd import poollib
    idx = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    rc = poollib.load().vboc_pool_select(sc._h, sd.data_ptr(), None, n, n + 1, 6, idx.data_ptr(), None, None, None,
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == poollib.EARG
    with pytest.raises(ValueError):
        sc.select(sd, Xd, n + 1)


@pytest.mark.gpu
def test_pool_ranking_against_the_reference_arithmetic():
    """70 001 rows, hidden 500, B = 1000: entropy64's docstring derives eps, ranking_ok's the two conditions."""
    model, mean, std = trained(6, 500)
    sc, X, Xd, etp, _ = scored(6, 500, 70001)
    r = sc.select(etp, Xd, 1000)
    e64, eps = entropy64(params64(model), X, mean, std)
    print("eps", eps)
    ranking_ok(e64, eps, r["idx"], 1000)
    # and the torch / scipy path of the same scorer class (the reference's arithmetic) obeys the same condition
    from vboc_amd.learn import PoolScorer
    ref = PoolScorer(3, model, None, "cuda", native=False)
    e_ref = ref.entropy(X, mean, std)
    assert np.abs(e_ref - etp.cpu().numpy()).max() <= 2 * eps
    ranking_ok(e64, eps, ref.select(e_ref, X, 1000)["idx"], 1000)


# -- the guess trajectories -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 17, 300])
@pytest.mark.parametrize("nin,hidden,N", [(6, 500, 100), (4, 300, 100), (2, 100, 5)])
def test_pool_guess_matches_float64_forward_and_nn_guess(nin, hidden, N, B):
    """Stages 1..N against the float64 forward of the same float32 parameters.  Bound: the network's output o has the
    module docstring's forward bound tau = c 2^-24 a3, c = nin + 2 H + 3; v = fl(o std) adds 2^-24 |o std| <= 2^-24 a3
    std, fl(v + mean) adds 2^-24 |v + mean| <= 2^-24 (a3 std + |mean|):
        bound = 2^-24 ((c + 2) a3 std + |mean|).
    al.nn_guess (torch, one row at a time, another summation order of the same operations) obeys the same bound
    against float64, so the two are within twice the bound of each other."""
    from vboc_amd.al import nn_guess
    from vboc_amd.learn import NeuralNetCLS, PoolScorer
    nq = nin // 2
    torch.manual_seed(7 * nin + N)
    g = NeuralNetCLS(nin, hidden, nin * N).cuda()
    cls = NeuralNetCLS(nin, hidden, 2).cuda()
    sc = PoolScorer(nq, cls, g, "cuda")
    X0 = pool_rows(nin, B, seed=B)
    mean, std = float(np.float32(1.3)), float(np.float32(5.1))
    xg = sc.guess(X0, N, mean, std)
    assert xg.shape == (B, N + 1, nin) and xg.dtype == torch.float64
    got = xg.cpu().numpy()
    assert np.array_equal(got[:, 0], X0)
    W = params64(g)
    out, a3 = forward64(W, norm32(X0, mean, std))
    c = nin + 2 * padded(hidden) + 3
    bound = U * ((c + 2) * a3 * std + abs(mean))
    want = out * np.float64(np.float32(std)) + np.float64(np.float32(mean))
    err = np.abs(got[:, 1:].reshape(B, -1) - want)
    print("guess error / bound", float((err / bound).max()))
    assert np.all(err <= bound)
    gc = NeuralNetCLS(nin, hidden, nin * N)
    gc.load_state_dict({k: v.cpu() for k, v in g.state_dict().items()})
    mt, st = torch.tensor(np.float32(mean)), torch.tensor(np.float32(std))
    for b in range(B):
        ref = nn_guess(N, X0[b, :nq], X0[b, nq:], gc, mt, st)
        assert np.array_equal(ref[0], got[b, 0])
        assert np.all(np.abs(ref[1:].reshape(-1) - got[b, 1:].reshape(-1)) <= 2 * bound[b])
    for b in sorted({0, min(16, B - 1), B - 1}):             # a row alone equals the row in the batch, bit for bit
        one = sc.guess(X0[b:b + 1], N, mean, std)
        assert torch.equal(one[0], xg[b])


@pytest.mark.gpu
def test_pool_unsupported_shapes_and_missing_parameters():
    from vboc_amd import poollib
    from vboc_amd.learn import NeuralNetCLS, PoolScorer
    lib = poollib.load()
    h = ctypes.c_void_p()
    assert lib.vboc_pool_create(6, 513, ctypes.byref(h)) == poollib.EUNSUPPORTED
    assert lib.vboc_pool_create(3, 100, ctypes.byref(h)) == poollib.EUNSUPPORTED
    with pytest.raises(ValueError):
        PoolScorer(3, NeuralNetCLS(6, 600, 2).cuda(), None, "cuda")
    sc = PoolScorer(3, NeuralNetCLS(6, 64, 2).cuda(), NeuralNetCLS(6, 64, 6 * 107).cuda(), "cuda")
    with pytest.raises(ValueError):
        sc.guess(pool_rows(6, 4, 0), 107, 0.0, 1.0)          # 642 outputs
    etp = torch.zeros(4, device="cuda")
    X = torch.zeros((4, 6), dtype=torch.float64, device="cuda")
    # raw pointers go to the library: another dtype, device or layout is refused before any launch
    for bad in (X.float(), X.cpu(), torch.zeros((4, 8), dtype=torch.float64, device="cuda")[:, :6], X[:, :4]):
        with pytest.raises(ValueError):
            sc.entropy(bad, 0.0, 1.0)
        with pytest.raises(ValueError):
            sc.select(etp, bad, 2)
    with pytest.raises(ValueError):
        sc.select(etp.double(), X, 2)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.vboc_pool_entropy(sc._h, X.data_ptr(), 4, 0.0, 1.0, etp.data_ptr(), None, None, s) == poollib.EARG
    assert b"set_classifier" in lib.vboc_pool_last_error()
