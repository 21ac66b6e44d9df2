"""Pruning on the native trainer (vboc_amd/csrc/fit.hip via learn.HipTrainer): the device-side magnitude selection
against torch's prune.global_unstructured, the masked Adam step against torch's reparametrised loop
(VBOC/vboc.py:564-625), and the forward-only evaluation kernel (RMSE, safety margin, :631-642).

Shapes: the three native ones at their smallest sizes, (nq 1, hidden 100, minibatch 32), (2, 300, 64), (3, 500, 64);
hidden 100 / 300 / 500 are padded to 128 / 320 / 512 in the trainer, so the padding is in play everywhere.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.utils.prune as prune

SHAPES = [(1, 100, 32), (2, 300, 64), (3, 500, 64)]
COUNT = {1: 10501, 2: 92101, 3: 254501}          # 2nq-hidden-1 parameter counts


def _features(n, nq, seed=0):
    from vboc_amd.learn import dir_features, position_stats
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(3 * np.pi / 4, 5 * np.pi / 4, (n, nq)), rng.uniform(-10, 10, (n, nq))]
    m, s = position_stats(X, nq)
    return dir_features(X, m, s, nq)


def _trainer(nq, hidden, k, seed=5, **kw):
    from vboc_amd.learn import HipTrainer
    return HipTrainer(nq, "cuda", hidden=hidden, minibatch=k, seed=seed, **kw)


def _targets(model):
    st = model.linear_relu_stack
    return tuple((st[i], name) for name in ("weight", "bias") for i in (0, 2, 4))


def _torch_masks(model, amount):
    """prune.global_unstructured on `model` (in place); the masks in parameter order."""
    prune.global_unstructured(_targets(model), pruning_method=prune.L1Unstructured, amount=amount)
    st = model.linear_relu_stack
    return [getattr(st[i], name + "_mask") for i in (0, 2, 4) for name in ("weight", "bias")]


def _mags(model):
    return torch.cat([p.detach().abs().flatten() for p in model.parameters()])


def _torch_steps(model, opt, F, nin, idx_steps, val, beta):
    crit = torch.nn.MSELoss()
    for idx in idx_steps:
        ii = torch.as_tensor(idx, dtype=torch.long, device="cuda")
        loss = crit(model(F[ii, :nin]), F[ii, nin:nin + 1])
        loss.backward()
        opt.step()
        opt.zero_grad()
        val = beta * val + (1 - beta) * loss.item()
    return val


def ref_margin(out, y):
    """VBOC/vboc.py:641 with the float32 output and the float64 target."""
    d = out.astype(np.float64) - y
    return float(np.amax(d[d > 0] / y[d > 0])) if (d > 0).any() else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("nq,hidden,k", SHAPES)
def test_selection_equals_torch_global_unstructured(nq, hidden, k):
    a = _trainer(nq, hidden, k)
    n = a.n_params()
    assert n == COUNT[nq]
    kk = round(0.5 * n)
    v = torch.sort(_mags(a.model)).values
    assert float(v[kk - 1]) < float(v[kk])                   # no tie decides
    ref = _torch_masks(copy.deepcopy(a.model), 0.5)
    assert a.prune(0.5) == kk
    masks = a.masks()
    for m, r in zip(masks, ref):
        assert torch.equal(m, r)
    assert sum(int((m == 0).sum()) for m in masks) == kk
    for p, m in zip(a.model.parameters(), masks):
        assert bool((p[m == 0] == 0).all()) and bool((p[m == 1] != 0).all())
    with pytest.raises(Exception):
        a.prune(0.5)                                         # a mask is active
    a.prune_remove()
    assert all(bool((m == 1).all()) for m in a.masks())
    assert sum(int((p == 0).sum()) for p in a.model.parameters()) == kk     # the zeros stay


@pytest.mark.gpu
@pytest.mark.parametrize("nq,hidden,k", SHAPES)
def test_selection_of_nothing_and_of_everything(nq, hidden, k):
    a = _trainer(nq, hidden, k)
    before = [p.detach().clone() for p in a.model.parameters()]
    assert a.prune(0.0) == 0
    assert all(bool((m == 1).all()) for m in a.masks())
    for p, q in zip(a.model.parameters(), before):
        assert torch.equal(p, q)
    b = _trainer(nq, hidden, k)
    assert b.prune(1.0) == COUNT[nq]
    assert all(bool((m == 0).all()) for m in b.masks())
    assert all(bool((p == 0).all()) for p in b.model.parameters())


@pytest.mark.gpu
@pytest.mark.parametrize("nq,hidden,k", SHAPES)
def test_selection_with_ties_is_exact_and_repeatable(nq, hidden, k):
    n = COUNT[nq]
    kk = n // 3
    got = []
    for _ in range(2):
        a = _trainer(nq, hidden, k)
        with torch.no_grad():
            w = a.model.linear_relu_stack[2].weight
            w.copy_(torch.where(w > 0, 0.5, -0.5))
        mags = [p.detach().abs().clone() for p in a.model.parameters()]
        assert a.prune(kk / n) == kk
        masks = a.masks()
        assert sum(int((m == 0).sum()) for m in masks) == kk
        pruned = torch.cat([g[m == 0] for g, m in zip(mags, masks)])
        kept = torch.cat([g[m == 1] for g, m in zip(mags, masks)])
        assert float(pruned.max()) <= float(kept.min())
        assert float(pruned.max()) == 0.5                    # the threshold sits on the tied value
        got.append(masks)
    for m0, m1 in zip(*got):
        assert torch.equal(m0, m1)


@pytest.mark.gpu
@pytest.mark.parametrize("nq,hidden,k", SHAPES)
def test_masked_steps_match_torch_reparametrised_loop(nq, hidden, k):
    Fn = _features(3000, nq, seed=nq)
    nin = 2 * nq
    F = torch.as_tensor(Fn, dtype=torch.float32, device="cuda")
    a = _trainer(nq, hidden, k)
    idx = _trainer(nq, hidden, k).sample(Fn.shape[0], 0, steps=8).cpu().numpy()
    ref = copy.deepcopy(a.model)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    val0 = float(Fn[:, nin].max())
    assert a.fit(Fn, it_max=4)["iterations"] == 3
    _torch_steps(ref, opt, F, nin, idx[:3], val0, a.beta)
    ref.load_state_dict(a.model.state_dict())               # both prune from identical values
    kk = round(0.5 * a.n_params())
    v = torch.sort(_mags(ref)).values
    assert float(v[kk - 1]) < float(v[kk])
    ref_masks = [m.clone() for m in _torch_masks(ref, 0.5)]
    assert a.prune(0.5) == kk
    for m, r in zip(a.masks(), ref_masks):
        assert torch.equal(m, r)
    r2 = a.fit(Fn, it_max=6)
    assert r2["iterations"] == 5
    v_ref = _torch_steps(ref, opt, F, nin, idx[3:8], val0, a.beta)
    for mod, name in _targets(ref):
        prune.remove(mod, name)
    assert abs(r2["val"] - v_ref) <= 1e-5 * abs(v_ref)
    for p, q, m in zip(a.model.parameters(), ref.parameters(), ref_masks):
        assert bool((p[m == 0] == 0).all()) and bool((q[m == 0] == 0).all())
        assert float((p.detach() - q.detach()).abs().max()) <= 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("nq,hidden,k", SHAPES)
def test_identity_mask_changes_nothing(nq, hidden, k):
    Fn = _features(3000, nq, seed=2)
    a, b = _trainer(nq, hidden, k, seed=7), _trainer(nq, hidden, k, seed=7)
    a.set_mask([torch.ones_like(p) for p in a.model.parameters()])
    ra, rb = a.fit(Fn, it_max=6), b.fit(Fn, it_max=6)
    assert ra["iterations"] == rb["iterations"] == 5 and ra["val"] == rb["val"]
    for p, q in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(p, q)
    for ma, mb in zip(a.moments(), b.moments()):
        for x, y in zip(ma, mb):
            assert torch.equal(x, y)


@pytest.mark.gpu
def test_graph_replay_equals_eager_under_a_mask():
    Fn = _features(3000, 3, seed=3)
    a = _trainer(3, 500, 64, seed=9, graphs=True, poll=64)
    b = _trainer(3, 500, 64, seed=9, graphs=False, poll=1)
    assert a.prune(0.5) == b.prune(0.5) == round(0.5 * COUNT[3])
    masks = a.masks()
    ra, rb = a.fit(Fn, it_max=130), b.fit(Fn, it_max=130)
    assert ra["iterations"] == rb["iterations"] == 129 and ra["val"] == rb["val"]
    assert ra["launched"] == 192 and rb["launched"] == 130
    for p, q, m in zip(a.model.parameters(), b.model.parameters(), masks):
        assert torch.equal(p, q)
        assert bool((p[m == 0] == 0).all())
    # the mask's removal is part of the graph key: the same trainer then trains the pruned entries again
    a.prune_remove()
    b.prune_remove()
    ra, rb = a.fit(Fn, it_max=130), b.fit(Fn, it_max=130)
    assert ra["iterations"] == rb["iterations"] == 129 and ra["val"] == rb["val"]
    for p, q in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(p, q)
    assert any(bool((p[m == 0] != 0).any()) for p, m in zip(a.model.parameters(), masks))


def _check_eval(tr, Fe):
    """evaluate(Fe) of the trainer's module against float64 / float32 torch forwards and NumPy statistics."""
    nin = tr.nin
    n = Fe.shape[0]
    x32 = torch.as_tensor(Fe[:, :nin], dtype=torch.float32, device="cuda")
    with torch.no_grad():
        ref64 = copy.deepcopy(tr.model).double()(x32.double())
        out_t = tr.model(x32)
    e1 = tr.evaluate(Fe)
    e2 = tr.evaluate(Fe)
    assert e1["out"].shape == (n, 1) and torch.equal(e1["out"], e2["out"])
    assert (e1["rmse"], e1["safety_margin"], e1["over"]) == (e2["rmse"], e2["safety_margin"], e2["over"])
    err_dev = float((e1["out"].double() - ref64).abs().max())
    err_t = float((out_t.double() - ref64).abs().max())
    print(f"n {n}: device error {err_dev:.3e}, torch float32 error {err_t:.3e}")
    assert err_dev <= max(4 * err_t, 1e-6), (err_dev, err_t)
    out = e1["out"].cpu().numpy()[:, 0]
    y = Fe[:, nin]
    rmse = float(np.sqrt(np.mean((out.astype(np.float64) - y) ** 2)))
    assert abs(e1["rmse"] - rmse) <= 1e-6 * rmse
    mg = ref_margin(out, y)
    assert abs(e1["safety_margin"] - mg) <= 1e-6 * abs(mg)
    assert e1["over"] == int((out.astype(np.float64) - y > 0).sum())
    assert tr.safety_margin(Fe) == e1["safety_margin"]
    return e1


@pytest.mark.gpu
@pytest.mark.parametrize("nq,hidden,k,n", [(1, 100, 32, 1007), (2, 300, 64, 1007), (3, 500, 64, 5),
                                           (3, 500, 64, 16), (3, 500, 64, 1007)])
def test_evaluate_forward_rmse_and_margin(nq, hidden, k, n):
    Fn = _features(3000, nq, seed=4)
    Fe = _features(n, nq, seed=8)
    Fe[:, 2 * nq] *= 0.05                                    # some outputs above their targets
    tr = _trainer(nq, hidden, k)
    tr.fit(Fn, it_max=41)
    e = _check_eval(tr, Fe)
    assert 0 < e["over"] <= n and e["safety_margin"] > 0
    # a float32 tensor: the float32 target column is promoted
    e32 = tr.evaluate(torch.as_tensor(Fe, dtype=torch.float32))
    assert torch.equal(e32["out"], e["out"])
    mg32 = ref_margin(e["out"].cpu().numpy()[:, 0], Fe[:, 2 * nq].astype(np.float32).astype(np.float64))
    assert abs(e32["safety_margin"] - mg32) <= 1e-6 * mg32
    # no output above its target, and no rows
    Fz = Fe.copy()
    Fz[:, 2 * nq] = 1e6
    ez = tr.evaluate(Fz)
    assert ez["safety_margin"] == 0.0 and ez["over"] == 0
    e0 = tr.evaluate(Fe[:0])
    assert (e0["rmse"], e0["safety_margin"], e0["over"]) == (0.0, 0.0, 0) and e0["out"].shape == (0, 1)
    # after a fit under a mask the packed weights carry the zeros: the outputs are the pruned module's
    tr.prune(0.5)
    tr.fit(Fn, it_max=11)
    assert sum(int((p == 0).sum()) for p in tr.model.parameters()) >= round(0.5 * COUNT[nq])
    _check_eval(tr, Fe)


@pytest.mark.gpu
def test_vboc_run_native_prunes_on_the_gpu_backend(tmp_path):
    from vboc_amd.drivers import GpuBackend
    from vboc_amd.learn import HipTrainer, dir_features
    from vboc_amd.pipeline import load_artifacts, make_test_set, vboc_run
    nq = 2
    be = GpuBackend(nq)
    X_test, _ = make_test_set(nq, be, num_prob=64, first_id=10**7)
    out = vboc_run(nq, be, X_test, stop_time=1e9, num_prob=64, max_iterations=1, out_dir=str(tmp_path),
                   trainer_kw=dict(native=True, minibatch=64, it_max=300), prune_amount=0.5)
    assert type(out["trainer"]) is HipTrainer
    assert out["prune"]["pruned"] == round(0.5 * COUNT[nq]) and 1 <= out["prune"]["fit"]["iterations"] < 300
    art = load_artifacts(str(tmp_path), nq)
    assert sum(int((p == 0).sum()) for p in art["model"].parameters()) == out["prune"]["pruned"]
    assert art["margin"] == out["safety_margin"]
    assert np.isfinite(out["prune"]["rmse"])
    # The restatement on the saved model, with its float64 forward: margin = max(0, max_i (o_i - y_i) / y_i), which
    # moves by at most max_i |delta o_i| / y_i when the outputs move by delta o.  The device outputs are within
    # E = max(4 x the error of torch's own float32 forward, 1e-6) of the float64 ones
    # (test_evaluate_forward_rmse_and_margin), so the margins agree within E / min y.
    F_test = dir_features(X_test, out["mean"], out["std"], nq)
    x32 = torch.as_tensor(F_test[:, :4], dtype=torch.float32)
    y = F_test[:, 4]
    with torch.no_grad():
        o32 = art["model"](x32).double().numpy()[:, 0]
        o64 = copy.deepcopy(art["model"]).double()(x32.double()).numpy()[:, 0]
    E = max(4 * float(np.abs(o32 - o64).max()), 1e-6)
    ref = max(0.0, float(np.max((o64 - y) / y)))
    print(f"margin {art['margin']:.9g}, float64 restatement {ref:.9g}, bound {E / y.min():.3e}")
    assert abs(art["margin"] - ref) <= E / y.min(), (art["margin"], ref, E, y.min())
