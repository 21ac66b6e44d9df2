"""pipeline.al_run(native_fit=True) on the GPU: the classifier's fits on csrc/cls.hip at the AL loop's widths (hidden
500 for the triple, 300 for the double with its split minibatch), inside test_al_loop's device-loop set-up: pool 4096,
N_init = B = 256, minibatch 64, it_max 20, two iterations on OCP<sys>INIT.
"""
import numpy as np
import pytest
import torch


@pytest.mark.gpu
@pytest.mark.parametrize("nq,hidden", [(3, 500), (2, 300)])
def test_al_run_fits_the_classifier_on_the_device(nq, hidden):
    from test_al_loop import _heldout, _pool
    from test_pool_device import entropy64, ranking_ok
    from vboc_amd.learn import HipClsTrainer
    from vboc_amd.pipeline import al_run
    n, B, k, seed = 4096, 256, 64, 3
    pool = _pool(nq, n, seed=40 + nq)
    X_test = _heldout(nq, m=50, seed=5)
    r = al_run(nq, X_test, pool=pool, B=B, N_init=B, hidden=hidden, minibatch=k, it_max=20, max_iterations=2,
               seed=seed, device="cuda", native_fit=True)
    tr = r["trainer"]
    assert r["native_fit"] is True and type(tr) is HipClsTrainer
    assert r["iterations"] == 2 and len(r["rmse"]) == 3
    # val from 1 stays above loss_stop = 0.1 for 21 steps (0.95 ** 21 > 0.34): every fit runs to `it <= it_max`
    assert r["split"]["fit_cls_steps"] == 3 * 21
    # the torch module follows each fit and is the handle's parameters
    fresh = HipClsTrainer(nq, "cuda", seed=seed, hidden=hidden, minibatch=k)
    final = {kk: v.detach().cpu() for kk, v in tr.model.state_dict().items()}
    chain = [{kk: v.detach().cpu() for kk, v in fresh.model.state_dict().items()}, *r["cls_states"], final]
    assert len(chain) == 4
    for a, b in zip(chain[:-1], chain[1:]):
        assert set(a) == set(b) and all(not torch.equal(a[kk], b[kk]) for kk in a)
    got = [torch.empty_like(p) for p in tr.model.parameters()]
    tr._cl.check(tr._lib.vboc_cls_get_params(tr._h, 0, *[t.data_ptr() for t in got], tr._stream()))
    for p, g in zip(tr.model.parameters(), got):
        assert torch.equal(p.detach(), g)
    # the queries against the float64 forward of the classifier as it stood
    cur = pool[B:]
    mean, std = float(r["mean"]), float(r["std"])
    for it in range(2):
        idx = r["queries"][it]
        assert idx.shape == (B,) and np.all(np.diff(idx) < 0)
        W = [r["cls_states"][it][kk].numpy().astype(np.float64) for kk in r["cls_states"][it]]
        e64, eps = entropy64(W, cur, mean, std)
        ranking_ok(e64, eps, idx, B)
        cur = np.delete(cur, idx, 0)
    # the last march read the module the last native fit wrote
    sc = r["scorer"]
    again = sc.boundary(sc.to_pool(X_test), r["mean"], r["std"], outward_dims=2 if nq == 3 else None)
    assert again["rmse"] == r["rmse"][-1]
    if nq == 2:
        # the sampler's stream advanced by one draw per step taken, and the refits drew split minibatches: a twin
        # moved to that position draws what the loop's handle draws next
        n_rows = r["X_iter"].shape[0]
        n_new = int((r["batches"][-1]["label"] != 2).sum())
        assert k // 2 <= n_new <= B and n_rows == 3 * B - r["dropped"]
        fresh.sample(n_rows, steps=r["split"]["fit_cls_steps"])
        a, b = fresh.sample(n_rows, steps=1, n_new=n_new), tr.sample(n_rows, steps=1, n_new=n_new)
        assert np.array_equal(a, b)
        assert a[0, :k // 2].max() < n_rows - n_new <= a[0, k // 2:].min() and len(np.unique(a)) == k
