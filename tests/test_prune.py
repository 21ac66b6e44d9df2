"""Pruning, the refit under the masks and the safety margin (vboc_amd.learn.DirTrainer, vboc_amd.pipeline) against
plain PyTorch / NumPy restatements of the reference's generic driver (VBOC/vboc.py:564-642)."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.utils.prune as prune

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def _data(n, nq, seed=0):
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(3 * np.pi / 4, 5 * np.pi / 4, (n, nq)), rng.uniform(-10, 10, (n, nq))]
    X[3, nq:] = 0.0
    return X


def _targets(model):
    """The reference's parameters_to_prune (VBOC/vboc.py:566-573)."""
    st = model.linear_relu_stack
    return tuple((st[i], name) for name in ("weight", "bias") for i in (0, 2, 4))


def _plain_loop(model, opt, gen, F, nq, k, it_max):
    """test_learn._plain_fit's loop (the reference's :596-616), on a given model / optimizer / generator."""
    crit = nn.MSELoss()
    Ft = torch.tensor(F, dtype=torch.float32)
    n = F.shape[0]
    it, val = 1, float(torch.tensor(max(F[:, 2 * nq]), dtype=torch.float32))
    while val > 1e-3 and it < it_max:
        idx = torch.topk(torch.rand(n, generator=gen), k, sorted=False).indices
        loss = crit(model(Ft[idx, :2 * nq]), Ft[idx, 2 * nq:])
        loss.backward()
        opt.step()
        opt.zero_grad()
        val = 0.95 * val + (1 - 0.95) * loss.item()
        it += 1
    return it


def _plain_prune_fit(seed, F, nq, hidden, k, it_max, amount):
    """Fit, prune.global_unstructured, refit with the same optimizer, prune.remove - in plain PyTorch, with the
    minibatch draws of DirTrainer's first and second fit."""
    from vboc_amd.learn import DirTrainer, NeuralNetDIR
    torch.manual_seed(seed)
    model = NeuralNetDIR(2 * nq, hidden, 1)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    _plain_loop(model, opt, torch.Generator().manual_seed(DirTrainer.fit_seed(seed, 1)), F, nq, k, it_max)
    prune.global_unstructured(_targets(model), pruning_method=prune.L1Unstructured, amount=amount)
    st = model.linear_relu_stack
    masks = [getattr(st[i], name + "_mask").clone() for i in (0, 2, 4) for name in ("weight", "bias")]
    _plain_loop(model, opt, torch.Generator().manual_seed(DirTrainer.fit_seed(seed, 2)), F, nq, k, it_max)
    for mod, name in _targets(model):
        prune.remove(mod, name)
    return model, masks


def ref_margin(out, y):
    """VBOC/vboc.py:641, the float64 reading: outputs[i] float32, X_test_dir[i][-1] float64."""
    out = np.asarray(out, dtype=np.float32).reshape(-1)
    r = [(np.float64(out[i]) - y[i]) / y[i] for i in range(len(y)) if np.float64(out[i]) - y[i] > 0]
    return float(np.amax(np.array(r)))


def test_dir_trainer_prune_refit_equals_plain_torch_loop():
    from vboc_amd.learn import DirTrainer, dir_features, position_stats
    nq, hidden, k = 3, 32, 128
    X = _data(3000, nq)
    m, s = position_stats(X, nq)
    F = dir_features(X, m, s, nq)
    tr = DirTrainer(nq, "cpu", hidden=hidden, minibatch=k, seed=5)
    n = tr.n_params()
    assert n == 6 * 32 + 32 + 32 * 32 + 32 + 32 + 1
    assert all(bool((mk == 1).all()) for mk in tr.masks())
    assert tr.fit(F, it_max=21)["iterations"] == 20
    assert tr.prune(0.5) == round(0.5 * n)
    assert tr.fit(F, it_max=21)["iterations"] == 20
    masks = tr.masks()
    tr.prune_remove()
    model, ref_masks = _plain_prune_fit(5, F, nq, hidden, k, 21, 0.5)
    for a, b in zip(masks, ref_masks):
        assert torch.equal(a, b)
    for a, b in zip(tr.model.parameters(), model.parameters()):
        np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), rtol=2e-4, atol=2e-6)
    assert [k_ for k_, _ in tr.model.named_parameters()] == [k_ for k_, _ in model.named_parameters()]
    assert sum(int((p == 0).sum()) for p in tr.model.parameters()) == round(0.5 * n)
    for p, mk in zip(tr.model.parameters(), masks):
        assert bool((p[mk == 0] == 0).all())
    assert all(bool((mk == 1).all()) for mk in tr.masks())
    # after prune.remove a fit trains every parameter again
    tr.fit(F, it_max=4)
    assert any(bool((p[mk == 0] != 0).any()) for p, mk in zip(tr.model.parameters(), masks))


def test_safety_margin_equals_the_reference_expression():
    from vboc_amd.learn import DirTrainer
    tr = DirTrainer(3, "cpu", hidden=16, minibatch=64, seed=2)
    rng = np.random.default_rng(1)
    F = rng.uniform(0.05, 1.0, (5000, 7))
    F[:, 6] = rng.uniform(0.01, 0.3, 5000)
    with torch.no_grad():
        tr.model.linear_relu_stack[4].bias.fill_(0.15)       # outputs on both sides of the targets
        out = tr.model(torch.Tensor(F[:, :6])).numpy()
    assert ((out[:, 0] - F[:, 6]) > 0).sum() > 10            # the case is not vacuous
    ref = ref_margin(out, F[:, 6])
    got = tr.safety_margin(F)
    assert isinstance(got, float) and abs(got - ref) <= 1e-6 * abs(ref), (got, ref)
    # no output above its target: 0.0 (the reference's np.amax of an empty array raises)
    F[:, 6] = 1e3
    assert tr.safety_margin(F) == 0.0


def test_vboc_run_prunes_and_saves_the_margin(tmp_path):
    from oracle_backend import OracleBackend
    from vboc_amd.learn import dir_features
    from vboc_amd.pipeline import load_artifacts, make_test_set, vboc_run
    nq = 2
    X_test, _ = make_test_set(nq, OracleBackend(nq), num_prob=8, out_dir=str(tmp_path))
    out = vboc_run(nq, OracleBackend(nq), X_test, stop_time=1e9, num_prob=6, max_iterations=1,
                   out_dir=str(tmp_path), trainer_kw=dict(hidden=16, minibatch=32), prune_amount=0.5)
    n = 4 * 16 + 16 + 16 * 16 + 16 + 16 + 1
    assert out["prune"]["amount"] == 0.5 and out["prune"]["pruned"] == round(0.5 * n)
    assert out["prune"]["fit"]["iterations"] >= 1 and np.isfinite(out["prune"]["rmse"])
    assert len(out["rmse"]) == 2                              # the loop's list is the unpruned fits'
    art = load_artifacts(str(tmp_path), nq)
    keys = [f"linear_relu_stack.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")]
    assert list(art["model"].state_dict()) == keys                 # no *_orig / *_mask left in the saved model
    assert sum(int((p == 0).sum()) for p in art["model"].parameters()) == round(0.5 * n)
    assert art["margin"] == out["safety_margin"]
    F_test = dir_features(X_test, out["mean"], out["std"], nq)
    with torch.no_grad():
        o = art["model"](torch.Tensor(F_test[:, :4])).numpy()
    if ((o[:, 0] - F_test[:, 4]) > 0).any():
        ref = ref_margin(o, F_test[:, 4])
        assert abs(art["margin"] - ref) <= 1e-6 * abs(ref)
    else:
        assert art["margin"] == 0.0
    # defaults: no pruning, the margin is still computed
    plain = tmp_path / "plain"
    out2 = vboc_run(nq, OracleBackend(nq), X_test, stop_time=1e9, num_prob=6, max_iterations=0,
                    out_dir=str(plain), trainer_kw=dict(hidden=16, minibatch=32))
    assert out2["prune"] is None and isinstance(out2["safety_margin"], float)
    assert load_artifacts(str(plain), nq)["margin"] == out2["safety_margin"]
