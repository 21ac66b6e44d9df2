"""The NN libraries (csrc/fit.hip, cls.hip, pool.hip) against the commit before their forward passes were shared
(nn_common.h's forward_rows / out_partials / out_sum and ray helpers, pool.hip's tile_gemm): every output array, bit for
bit.  tests/golden/nn_parent.json holds the sha1 (and, for diagnosis, the first 8 values) of each array, recorded on an
MI355X from the parent commit's libraries by tools/record_nn_parent.py, which runs the case functions of this module;
the test runs them on the tree's libraries.  Every kernel involved has fixed reduction orders, so the hashes repeat.

Inputs and weights come from seeded NumPy generators (uniform draws only), never from a trained model, so they do not
depend on a card or on torch's CPU kernels.  Cases (each well under a second):

  pool entropy   hidden 64, 100, 200, 300, 500 (NT 1, 2, 4, 5, 8) at inputs 6, inputs 2 and 4 at hidden 300; 197 rows
                 (three full 64-row tiles and a partial, clamped one): etp, logits, labels.  One case of 2048 * 64 + 70
                 rows, where a workgroup runs a second round.
  pool guess     inputs 6, hidden 300, N = 5, 37 states.
  pool march     (inputs, hidden, outward_dims) = (4, 100, 0), (4, 300, 0), (6, 100, 2), (6, 300, 2), (6, 100, 0); 24 rays,
                 max_steps 200 (four rounds of 64, the last one short) under a classifier with label 1 inside an L1 ball
                 of radius 1.5 around velocity 3 e_last, over small random weights everywhere else: rays that take no
                 step, end on the norm around the first round's edge and in the third round, end on a label change from
                 either label, and end on max_steps from either label (_march_rays).
  cls            inputs 2, 4, 6, hidden 100, minibatch 32: five steps eager and five in a graph (parameters, both
                 moments, val), eval on 37 rows (two blocks and a partial one), boundary on 16 rays (inputs 4, 6).
  fit            (nq, hidden, minibatch) = (1, 100, 32), (2, 300, 64), (3, 500, 64): five steps with n_new = 0, five
                 with n_new > 0, five under a 50 % mask (parameters, moments, val), evaluate on 37 rows.
"""
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nn_parent.json")
MEAN, STD = 0.25, 2.0             # exact in float32
Q_LO, Q_HI = 3 * np.pi / 4, 5 * np.pi / 4

ENTROPY = [(6, 64), (6, 100), (6, 200), (6, 300), (6, 500), (2, 300), (4, 300)]
MARCH = [(4, 100, 0), (4, 300, 0), (6, 100, 2), (6, 300, 2), (6, 100, 0)]
FIT = [(1, 100, 32), (2, 300, 64), (3, 500, 64)]


def _fill(model, seed, last_bias=0.0):
    """Every parameter from uniform(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) of a NumPy generator, in parameter order."""
    import torch
    rng = np.random.default_rng(seed)
    ps = list(model.parameters())
    with torch.no_grad():
        for w, b in zip(ps[0::2], ps[1::2]):
            k = 1.0 / np.sqrt(w.shape[1])
            w.copy_(torch.from_numpy(rng.uniform(-k, k, tuple(w.shape)).astype(np.float32)))
            b.copy_(torch.from_numpy(rng.uniform(-k, k, tuple(b.shape)).astype(np.float32)))
        ps[-1].add_(last_bias)
    return model


def _states(n, nq, seed, vmax=10.0):
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(Q_LO, Q_HI, (n, nq)), rng.uniform(-vmax, vmax, (n, nq))]


def _cls_model(nin, hidden, outputs, seed):
    from vboc_amd.learn import NeuralNetCLS
    return _fill(NeuralNetCLS(nin, hidden, outputs), seed).cuda()


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------
# the cases: each returns {array name: NumPy array}
# ---------------------------------------------------------------------------------------------------------------
def _entropy(sc, X):
    """vboc_pool_entropy with all three outputs on the scorer's handle."""
    import torch
    Xd = sc.to_pool(X)
    n = Xd.shape[0]
    etp = torch.empty((n,), dtype=torch.float32, device="cuda")
    lg = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    lab = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    sc._pl.check(sc._lib.vboc_pool_set_classifier(sc._h, *sc._ptrs(sc.cls_model), sc._stream()))
    sc._pl.check(sc._lib.vboc_pool_entropy(sc._h, Xd.data_ptr(), n, MEAN, STD, etp.data_ptr(), lg.data_ptr(),
                                           lab.data_ptr(), sc._stream()))
    torch.cuda.synchronize()
    return dict(etp=_np(etp), logits=_np(lg), labels=_np(lab))


def case_pool_entropy(nin, hidden, n=197):
    from vboc_amd.learn import PoolScorer
    sc = PoolScorer(nin // 2, _cls_model(nin, hidden, 2, seed=100 + nin + hidden), None, "cuda")
    return _entropy(sc, _states(n, nin // 2, seed=nin * hidden + n))


def case_pool_entropy_second_round():
    return case_pool_entropy(6, 300, n=2048 * 64 + 70)


def case_pool_guess():
    from vboc_amd.learn import PoolScorer
    nin, hidden, N, B = 6, 300, 5, 37
    sc = PoolScorer(3, _cls_model(nin, hidden, 2, seed=1), _cls_model(nin, hidden, nin * N, seed=2), "cuda")
    xg = sc.guess(_states(B, 3, seed=3), N, MEAN, STD)
    return dict(x_guess=_np(xg))


def _ball_model(nin, hidden):
    """NeuralNetCLS(nin, hidden, 2): logit0 = sum_i |v_i - c_i|, logit1 = 1.5 with c = 3 e_last (label 1 inside that L1
    ball), on hidden units relu(+-(v_i - c_i)) passed through the second layer - plus uniform(-0.005, 0.005) on every
    parameter, so that every product of the forward pass has non-trivial operands."""
    import torch
    from vboc_amd.learn import NeuralNetCLS
    nq = nin // 2
    rng = np.random.default_rng(7 * nin + hidden)
    model = NeuralNetCLS(nin, hidden, 2)
    st = model.linear_relu_stack
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.from_numpy(rng.uniform(-0.005, 0.005, tuple(p.shape)).astype(np.float32)))
        for i in range(nq):
            ci = 3.0 if i == nq - 1 else 0.0
            for sgn, row in ((1.0, i), (-1.0, nq + i)):         # relu(sgn (STD xhat_i + MEAN - c_i))
                st[0].weight[row, nq + i] += sgn * STD
                st[0].bias[row] += sgn * (MEAN - ci)
                st[2].weight[row, row] += 1.0
                st[4].weight[0, row] += 1.0
        st[4].bias[1] += 1.5
    return model.cuda()


def _march_rays(nq):
    """24 held-out states.  a: the velocity components before the last one, z: the last one."""
    rng = np.random.default_rng(50 + nq)
    d = np.array([0.6, -0.8])[:nq - 1] if nq == 3 else np.array([1.0])
    flat = lambda s: np.r_[s * d, 0.0]                            # label 0 all the way to the origin
    near = lambda z: np.r_[np.array([0.05, 0.02])[:nq - 1], z]    # on the ball's axis
    V = [flat(0.005), flat(-0.004), np.r_[np.zeros(nq - 1), 0.006]]                       # 0..2: no step
    V += [flat(s) for s in (0.63, 0.64, 0.65, 0.66, 0.67, 1.5)]                           # 3..8: end on the norm
    V += [flat(2.5), flat(3.0)]                                                           # 9, 10: label 0, max_steps
    V += [near(4.0), near(4.2), near(3.9)]                                                # 11..13: label 1, leaves the ball
    V += [near(2.0), near(1.8)]                                                           # 14, 15: label 1, max_steps
    V += [near(5.0), near(5.5), near(4.6)]                                                # 16..18: label 0, enters the ball
    V += [np.r_[np.array([0.004, -0.003])[:nq - 1], 3.0], np.r_[np.array([0.0, 0.006])[:nq - 1], 2.5]]   # 19, 20
    V += [rng.uniform(-4.0, 4.0, nq) for _ in range(3)]                                   # 21..23
    V = np.array(V)
    assert V.shape == (24, nq)
    return np.c_[rng.uniform(Q_LO, Q_HI, (24, nq)), V]


def case_pool_march(nin, hidden, od):
    from vboc_amd.learn import PoolScorer
    sc = PoolScorer(nin // 2, _ball_model(nin, hidden), None, "cuda")
    b = sc.boundary(_march_rays(nin // 2), MEAN, STD, max_steps=200, outward_dims=od)
    return dict(err=b["err"], steps=b["steps"], flags=b["flags"])


def _cls_rows(n, nq, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.5, 1.5, (n, 2 * nq))
    inside = np.sum(np.abs(X[:, nq:]), axis=1) < 0.8 * nq
    return np.c_[X, ~inside, inside].astype(np.float32)


def _train_out(tr, r):
    out = {f"p{i}": _np(p) for i, p in enumerate(tr.model.parameters())}
    for name, ts in zip(("m", "v"), tr.moments()):
        out.update({f"{name}{i}": _np(t) for i, t in enumerate(ts)})
    out["val"] = np.array([r["val"]], dtype=np.float64)
    out["iterations"] = np.array([r["iterations"]], dtype=np.int64)
    return out


def case_cls_train(nq, graphs):
    from vboc_amd.learn import HipClsTrainer
    tr = HipClsTrainer(nq, "cuda", graphs=graphs, poll=64 if graphs else 1, hidden=100, minibatch=32, stop_val=0.0,
                       seed=11)
    _fill(tr.model, seed=20 + nq)
    return _train_out(tr, tr.fit(_cls_rows(500, nq, seed=30 + nq), it_max=5))


def _cls_fresh(nq):
    from vboc_amd.learn import HipClsTrainer
    tr = HipClsTrainer(nq, "cuda", hidden=100, minibatch=32, seed=11)
    _fill(tr.model, seed=40 + nq)
    return tr


def case_cls_eval(nq):
    tr = _cls_fresh(nq)
    lab, cnt, lg = tr.predict_labels(_cls_rows(37, nq, seed=60 + nq)[:, :2 * nq], logits=True)
    return dict(labels=_np(lab), count=np.array([cnt], dtype=np.int64), logits=_np(lg))


def case_cls_boundary(nq):
    tr = _cls_fresh(nq)
    X = _states(16, nq, seed=70 + nq, vmax=3.0)
    X[0, nq:] = 0.004            # no step
    X[1, nq:] *= 0.1             # a short ray
    b = tr.boundary_errors(X, MEAN, STD, max_steps=100)
    return dict(err=b["err"], steps=b["steps"], flags=b["flags"])


def _fit_rows(n, nq, seed):
    """[n, 2nq + 1] float64: inputs, then a positive target."""
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(-1.5, 1.5, (n, 2 * nq)), rng.uniform(0.2, 3.0, (n, 1))]


def _fit_trainer(nq, hidden, k):
    from vboc_amd.learn import HipTrainer
    tr = HipTrainer(nq, "cuda", hidden=hidden, minibatch=k, seed=5, stop_val=0.0)
    _fill(tr.model, seed=80 + nq, last_bias=0.5)          # most rows pass the last ReLU
    return tr


def case_fit_train(nq, hidden, k, mode):
    tr = _fit_trainer(nq, hidden, k)
    F = _fit_rows(400, nq, seed=90 + nq)
    if mode == "mask":
        tr.prune(0.5)
    return _train_out(tr, tr.fit(F, n_new=100 if mode == "refit" else 0, it_max=5))


def case_fit_eval(nq, hidden, k):
    tr = _fit_trainer(nq, hidden, k)
    e = tr.evaluate(_fit_rows(37, nq, seed=95 + nq))
    return dict(out=_np(e["out"]), rmse=np.array([e["rmse"]]), margin=np.array([e["safety_margin"]]),
                over=np.array([e["over"]], dtype=np.int64))


CASES = {}
for _nin, _h in ENTROPY:
    CASES[f"pool_entropy-{_nin}-{_h}"] = (case_pool_entropy, (_nin, _h))
CASES["pool_entropy_second_round"] = (case_pool_entropy_second_round, ())
CASES["pool_guess"] = (case_pool_guess, ())
for _nin, _h, _od in MARCH:
    CASES[f"pool_march-{_nin}-{_h}-od{_od}"] = (case_pool_march, (_nin, _h, _od))
for _nq in (1, 2, 3):
    CASES[f"cls_train-{_nq}-eager"] = (case_cls_train, (_nq, False))
    CASES[f"cls_train-{_nq}-graph"] = (case_cls_train, (_nq, True))
    CASES[f"cls_eval-{_nq}"] = (case_cls_eval, (_nq,))
for _nq in (2, 3):
    CASES[f"cls_boundary-{_nq}"] = (case_cls_boundary, (_nq,))
for _nq, _h, _k in FIT:
    for _mode in ("first", "refit", "mask"):
        CASES[f"fit_train-{_nq}-{_mode}"] = (case_fit_train, (_nq, _h, _k, _mode))
    CASES[f"fit_eval-{_nq}"] = (case_fit_eval, (_nq, _h, _k))
HASH_ONLY = ("pool_entropy_second_round",)


def digest(arrays):
    """{name: {sha1, dtype, shape, head}} of a case's arrays."""
    out = {}
    for k, a in arrays.items():
        a = np.ascontiguousarray(a)
        out[k] = dict(sha1=hashlib.sha1(a.tobytes()).hexdigest(), dtype=str(a.dtype), shape=list(a.shape),
                      head=[float(v) for v in a.reshape(-1)[:8]])
    return out


def run_case(name):
    fn, args = CASES[name]
    return fn(*args)


# ---------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_holds_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    for name in HASH_ONLY:
        assert all("head" not in v for v in golden["cases"][name].values())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bit_for_bit_against_the_parent(golden, name):
    got, want = digest(run_case(name)), golden["cases"][name]
    assert sorted(got) == sorted(want)
    bad = []
    for k in got:
        assert got[k]["dtype"] == want[k]["dtype"] and got[k]["shape"] == want[k]["shape"], k
        if got[k]["sha1"] != want[k]["sha1"]:
            bad.append(k)
            print(f"{name} {k}: head {got[k]['head']} parent {want[k].get('head')}")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("nin,hidden,od", MARCH)
def test_march_rays_end_in_every_way(nin, hidden, od):
    """Conditions on the march case's inputs: what the 24 rays are there for does happen."""
    r = case_pool_march(nin, hidden, od)
    steps, flags, err = r["steps"], r["flags"], r["err"]
    lab, capped = flags & 1, (flags >> 1) & 1
    print(steps.tolist(), flags.tolist())
    assert (steps[:3] == 0).all() and (err[:3] == 0).all()
    s = np.array([0.63, 0.64, 0.65, 0.66, 0.67, 1.5])
    assert (lab[3:9] == 0).all() and not capped[3:9].any() and (np.abs(steps[3:9] - 100 * s) <= 1).all()
    assert (err[3:9] >= s - 0.0101).all()                         # the last point's norm is not > 1e-2
    assert {63, 64, 65} & set(steps[3:8].tolist()) and (steps[8] - 1) // 64 == 2
    assert (steps[9:11] == 200).all() and (flags[9:11] == 2).all()
    assert (lab[11:14] == 1).all() and not capped[11:14].any() and (steps[11:14] < 100).all()
    assert (steps[14:16] == 200).all() and (flags[14:16] == 3).all()
    assert (lab[16:19] == 0).all() and not capped[16:19].any() and (err[16:19] < 1.2).all()      # far from the origin
    assert (lab[19:21] == 1).all()
    if od == 2:
        assert (steps[19:21] == 0).all()                          # the first two components alone decide
    else:
        assert (steps[19:21] > 0).all()
