"""The classifier's training step at the AL loop's widths (vboc_amd/csrc/cls.hip at <4, 320> and <6, 512>: hidden 300
and 500) and the split minibatch on the classifier's ABI (vboc_cls_train_split / vboc_cls_sample_split).

CPU: the symbols, clslib.fit_supported's truth table, the wide instantiations in the gfx950 code object, the CPU
fall-backs of make_cls_trainer and al_run(native_fit=True).  GPU: the fit against torch.optim.Adam + BCEWithLogitsLoss
on the sampler's own indices at the bars of test_fit_device.test_device_fit_matches_torch_adam_loop (measured for
fit.hip at these widths, reused by test_cls_device at 128), with and without a split minibatch; the sampler; graph
replay against eager launches; the padding; the refusals; and the accuracy after 300 steps against ClsTrainer's own
spread over five seeds.
"""
import copy
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N_ROWS = 30000
WIDE = {3: 500, 2: 300}


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_split_entries_are_declared_listed_and_exported():
    from vboc_amd import clslib
    hdr = open(os.path.join(HERE, "..", "include", "vboc_cls.h")).read()
    declared = set(re.findall(r"\b(vboc_cls_\w+)\s*\(", hdr))
    lib = ctypes.CDLL(clslib.LIB_PATH)
    for name in ("vboc_cls_train_split", "vboc_cls_sample_split"):
        assert name in declared and name in clslib.EXPORTS
        getattr(lib, name)


def test_fit_supported_truth_table():
    from vboc_amd.clslib import fit_supported, supported
    for nin, hidden in [(6, 500), (6, 449), (6, 512), (4, 300), (4, 257), (4, 320), (2, 100), (4, 100), (6, 100)]:
        assert fit_supported(nin, hidden, 4096) and fit_supported(nin, hidden, 64), (nin, hidden)
    for nin, hidden in [(6, 448), (6, 513), (4, 321), (4, 256), (6, 300), (2, 300)]:
        assert not fit_supported(nin, hidden, 4096), (nin, hidden)
    for nin, hidden in [(6, 500), (4, 300), (6, 100)]:
        assert not fit_supported(nin, hidden, 8192) and not fit_supported(nin, hidden, 48)
    assert not supported(6, 500, 4096) and not supported(4, 300, 4096) and supported(6, 100, 4096)


def test_code_object_holds_the_wide_training_kernels():
    from vboc_amd import clslib
    sys.path.insert(0, os.path.join(HERE, "..", "tools"))
    try:
        from kernel_digest import digests
    finally:
        sys.path.pop(0)
    names = list(digests(clslib.LIB_PATH))
    for kernel in ("k_fwd_bwd", "k_dw1", "k_adam", "k_pack"):
        for nin, hp in ((4, 320), (6, 512), (2, 128), (4, 128), (6, 128)):
            tag = f"{len(kernel)}{kernel}ILi{nin}ELi{hp}EE"
            assert any(tag in n for n in names), tag
    # the forward-only kernels exist at 128 alone: one instantiation per input count
    assert sum("k_eval" in n for n in names) == 3 and sum("k_boundary" in n for n in names) == 2


def test_make_cls_trainer_keeps_torch_on_the_cpu_at_the_wide_shapes():
    from vboc_amd.learn import ClsTrainer, make_cls_trainer
    assert type(make_cls_trainer(3, "cpu", native=True, hidden=500)) is ClsTrainer
    assert type(make_cls_trainer(2, "cpu", native=True, hidden=300)) is ClsTrainer


@pytest.mark.parametrize("nq", [3, 2])
def test_al_run_native_fit_on_the_cpu_is_the_torch_run(nq):
    """On the CPU native_fit=True falls back to ClsTrainer (make_trainer's rule): the same run bit for bit, at a shape
    the device library would train."""
    from test_al_loop import _stub_run
    kw = dict(n=200, hidden=WIDE[nq], minibatch=32, it_max=2, max_iterations=2)
    a = _stub_run(nq, [0.5], native_fit=True, **kw)
    b = _stub_run(nq, [0.5], **kw)
    assert a["native_fit"] is False and b["native_fit"] is False
    assert a["iterations"] == b["iterations"] == 2 and a["split"]["fit_cls_steps"] == 3 * 3
    for key in ("trainer", "guess_trainer"):
        sa, sb = a[key].model.state_dict(), b[key].model.state_dict()
        assert set(sa) == set(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (key, k)
    assert len(a["queries"]) == len(b["queries"]) == 2
    for qa, qb in zip(a["queries"], b["queries"]):
        assert np.array_equal(qa, qb)
    assert np.array_equal(a["rmse"], b["rmse"], equal_nan=True) and np.array_equal(a["X_iter"], b["X_iter"])


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
_ROWS = {}


def _data(nq, speed=None):
    """test_cls_device._rows with 30 000 rows, made once per (nq, speed) and left unchanged."""
    from test_cls_device import _rows
    if (nq, speed) not in _ROWS:
        _ROWS[nq, speed] = _rows(N_ROWS, nq, seed=20 + nq, speed=speed)[0].cuda()
    return _ROWS[nq, speed]


def _check_fit(nq, k, n_new):
    """One step, then four more, against torch on the indices a twin of the same seed draws."""
    from test_cls_device import _torch_steps
    from vboc_amd.learn import HipClsTrainer
    n, nin, hidden = N_ROWS, 2 * nq, WIDE[nq]
    F = _data(nq)
    a = HipClsTrainer(nq, "cuda", seed=5, hidden=hidden, minibatch=k)
    twin = HipClsTrainer(nq, "cuda", seed=5, hidden=hidden, minibatch=k)
    idx = twin.sample(n, steps=5, n_new=n_new)
    assert idx.shape == (5, k) and all(len(np.unique(r)) == k for r in idx)
    if n_new:
        assert idx[:, :k // 2].max() < n - n_new <= idx[:, k // 2:].min() and idx.max() < n
    ref = copy.deepcopy(a.model)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    r1 = a.fit(F, it_max=1, n_new=n_new)
    assert r1["iterations"] == 1
    v_ref = _torch_steps(ref, opt, F, nin, idx[:1], 1.0, a.beta)
    m_dev, v_dev = a.moments()
    worst = dict(exp_avg=0.0, exp_avg_sq=0.0, param1=0.0, param5=0.0, val=0.0)
    for p, md, vd in zip(ref.parameters(), m_dev, v_dev):
        mr, vr = opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
        em = float((md - mr).abs().max()) / (float(mr.abs().max()) + 1e-30)
        ev = float((vd - vr).abs().max()) / (float(vr.abs().max()) + 1e-30)
        worst["exp_avg"], worst["exp_avg_sq"] = max(worst["exp_avg"], em), max(worst["exp_avg_sq"], ev)
    worst["val"] = abs(r1["val"] - v_ref) / abs(v_ref)
    worst["param1"] = max(float((p - q).detach().abs().max()) for p, q in zip(a.model.parameters(), ref.parameters()))
    r2 = a.fit(F, it_max=4, n_new=n_new)
    assert r2["iterations"] == 4
    v_ref = _torch_steps(ref, opt, F, nin, idx[1:5], 1.0, a.beta)
    worst["val"] = max(worst["val"], abs(r2["val"] - v_ref) / abs(v_ref))
    worst["param5"] = max(float((p - q).detach().abs().max()) for p, q in zip(a.model.parameters(), ref.parameters()))
    print("measured", (nq, hidden, k, n_new), {kk: f"{v:.3g}" for kk, v in worst.items()})
    assert worst["exp_avg"] <= 2e-5, worst
    assert worst["exp_avg_sq"] <= 5e-5, worst
    assert worst["param1"] <= 1e-5, worst
    assert worst["param5"] <= 2e-5, worst
    assert worst["val"] <= 1e-5, worst


@pytest.mark.gpu
@pytest.mark.parametrize("nq,k", [(3, 64), (3, 4096), (2, 64), (2, 4096)])
def test_wide_cls_fit_matches_torch_adam_bce_loop(nq, k):
    """(nq 3, hidden 500) and (nq 2, hidden 300) at minibatch 64 (S = 2) and 4096 (S = 4 at HP 512, S = 8 with k_dw1's
    5 x 5 blocks at HP 320).  Measured on an MI355X, as a share of each bar: see DESIGN section 21."""
    _check_fit(nq, k, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [64, 4096])
def test_wide_cls_fit_with_a_split_minibatch_matches_torch(k):
    """n_new = 12 000 of 30 000 rows: the twin's draws are split at row 18 000, and the fit matches torch on them, so the
    training path draws through the split sampler."""
    _check_fit(2, k, 12000)


@pytest.mark.gpu
def test_cls_sampler_is_a_uniform_subset_of_each_range():
    """test_fit_device.test_sampler_is_a_uniform_subset_of_each_range's cases and chi-square bound on the classifier's
    ABI; n_new = 0 is vboc_cls_sample."""
    from vboc_amd.learn import HipClsTrainer
    tr = HipClsTrainer(1, "cuda", seed=1, hidden=100, minibatch=32)
    for n, n_new, steps in [(100, 0, 3000), (40, 0, 3000), (100, 40, 3000), (80, 30, 3000)]:
        idx = tr.sample(n, steps=steps, n_new=n_new)
        assert idx.min() >= 0 and idx.max() < n
        assert all(len(np.unique(r)) == 32 for r in idx)
        parts = [(0, n, 32)] if not n_new else [(0, n - n_new, 16), (n - n_new, n, 16)]
        for c, (lo, hi, kk) in enumerate(parts):
            sub = idx[:, c * kk:(c + 1) * kk] if n_new else idx
            assert sub.min() >= lo and sub.max() < hi
            cnt = np.bincount(sub.ravel() - lo, minlength=hi - lo)
            e = steps * kk / (hi - lo)
            chi2 = float(((cnt - e) ** 2 / e).sum())
            dof = hi - lo - 1
            assert chi2 < dof + 6 * np.sqrt(2 * dof), (n, n_new, chi2, dof)
    a = HipClsTrainer(1, "cuda", seed=7, hidden=100, minibatch=32)
    b = HipClsTrainer(1, "cuda", seed=7, hidden=100, minibatch=32)
    new = a.sample(1000, steps=6, n_new=0)
    old = torch.empty((6, 32), dtype=torch.int32, device="cuda")
    b._cl.check(b._lib.vboc_cls_sample(b._h, 1000, 6, old.data_ptr(), b._stream()))
    assert np.array_equal(new, old.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("nq,n_new", [(3, 0), (2, 8000)])
def test_wide_cls_graph_replay_equals_eager_and_stops_exactly(nq, n_new):
    """poll-64 graph replays == step-by-step launches, bit for bit, on a run that stops on val: one class."""
    from vboc_amd.learn import HipClsTrainer
    F = _data(nq).clone()
    F[:, 2 * nq], F[:, 2 * nq + 1] = 1.0, 0.0
    a = HipClsTrainer(nq, "cuda", seed=9, hidden=WIDE[nq], graphs=True, poll=64)
    b = HipClsTrainer(nq, "cuda", seed=9, hidden=WIDE[nq], graphs=False, poll=1)
    ra, rb = a.fit(F, it_max=5000, n_new=n_new), b.fit(F, it_max=5000, n_new=n_new)
    assert ra["iterations"] == rb["iterations"] < 5000, (ra, rb)
    assert ra["val"] == rb["val"] and ra["val"] <= 5e-3
    assert rb["launched"] == rb["iterations"] + 1 and ra["launched"] % 64 == 0
    for p, q in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(p, q)


@pytest.mark.gpu
@pytest.mark.parametrize("nq,full,live", [(3, 512, 500), (2, 320, 300)])
def test_wide_cls_zero_hidden_units_stay_exactly_zero(nq, full, live):
    """A twin at the padded width whose units live.. are zero, as the padding of the AL width is: after 50 steps the
    parameters and both Adam moments of those units are still exactly zero, and the live block is not."""
    from vboc_amd.learn import HipClsTrainer
    a = HipClsTrainer(nq, "cuda", seed=2, hidden=full, stop_val=0.0)
    st = a.model.linear_relu_stack
    with torch.no_grad():
        st[0].weight[live:] = 0
        st[0].bias[live:] = 0
        st[2].weight[live:] = 0
        st[2].weight[:, live:] = 0
        st[2].bias[live:] = 0
        st[4].weight[:, live:] = 0
    assert a.fit(_data(nq), it_max=50)["iterations"] == 50
    for ts in [list(a.model.parameters())] + a.moments():
        W0, b0, W1, b1, W2, b2 = ts
        for t in (W0[live:], b0[live:], W1[live:], W1[:, live:], b1[live:], W2[:, live:]):
            assert float(t.detach().abs().max()) == 0.0
        assert float(W1[:live, :live].detach().abs().max()) > 0.0


def _params(tr, which=0):
    ts = [torch.empty_like(p) for p in tr.model.parameters()]
    tr._cl.check(tr._lib.vboc_cls_get_params(tr._h, which, *[t.data_ptr() for t in ts], tr._stream()))
    torch.cuda.synchronize()
    return ts


@pytest.mark.gpu
def test_wide_cls_refusals_write_nothing_and_leave_the_handle_usable():
    from vboc_amd import clslib
    from vboc_amd.learn import HipClsTrainer
    EARG, EUNS = -1, clslib.EUNSUPPORTED
    nq, k, n = 3, 64, N_ROWS
    F = _data(nq)
    tr = HipClsTrainer(nq, "cuda", seed=4, hidden=500, minibatch=k)
    lib, h, s = tr._lib, tr._h, tr._stream()
    tr._push()
    before = [_params(tr, w) for w in (0, 1, 2)]
    its = ctypes.c_longlong(-5)
    run = clslib.ClsRun(F=F.data_ptr(), n=n, ld=F.shape[1], it_max=3, val0=1.0, stop_val=0.0, beta=0.95, lr=1e-3,
                        poll=1, graphs=0, iterations=ctypes.addressof(its), val=None, launched=None, kernel_ms=None)
    sentinel = torch.full((k,), -7, dtype=torch.int32, device="cuda")
    for n_new in (-1, n + 1, k // 2 - 1, n - k // 2 + 1):
        assert lib.vboc_cls_train_split(h, ctypes.byref(run), n_new, s) == EARG, n_new
        assert lib.vboc_cls_sample_split(h, n, n_new, 1, sentinel.data_ptr(), s) == EARG, n_new
    # forward-only calls on a wide handle
    X = F[:100, :6].contiguous()
    lab = torch.full((100,), 9, dtype=torch.uint8, device="cuda")
    lg = torch.full((100, 2), -7.0, device="cuda")
    cnt = ctypes.c_longlong(-5)
    assert lib.vboc_cls_eval(h, X.data_ptr(), 100, 6, lab.data_ptr(), lg.data_ptr(), ctypes.byref(cnt), s) == EUNS
    Xt = torch.rand((10, 6), dtype=torch.float64, device="cuda")
    err = torch.full((10,), -7.0, dtype=torch.float64, device="cuda")
    steps = torch.full((10,), -7, dtype=torch.int32, device="cuda")
    flags = torch.full((10,), 9, dtype=torch.uint8, device="cuda")
    assert lib.vboc_cls_boundary(h, Xt.data_ptr(), 10, 3, 0.0, 1.0, 0, err.data_ptr(), steps.data_ptr(),
                                 flags.data_ptr(), s) == EUNS
    torch.cuda.synchronize()
    assert its.value == -5 and cnt.value == -5
    assert bool((sentinel == -7).all()) and bool((lab == 9).all()) and bool((lg == -7.0).all())
    assert bool((err == -7.0).all()) and bool((steps == -7).all()) and bool((flags == 9).all())
    for w, ts in zip((0, 1, 2), before):
        for t, u in zip(ts, _params(tr, w)):
            assert torch.equal(t, u)
    # unsupported shapes: no handle
    for nin, hidden in ((6, 448), (6, 513), (4, 321)):
        out = ctypes.c_void_p(1)
        assert lib.vboc_cls_create(nin, hidden, 4096, 0, ctypes.byref(out)) == EUNS and not out.value
    # the handle still fits, and the torch path still classifies
    assert tr.fit(F, it_max=3)["iterations"] == 3
    assert any(not torch.equal(t, u) for t, u in zip(before[0], _params(tr, 0)))
    lab2, cnt2 = tr.predict_labels(X)
    assert lab2.shape == (100,) and 0 <= cnt2 <= 100


@pytest.mark.gpu
def test_wide_cls_learns_like_the_torch_trainer():
    """300 steps at (3, 500, 4096) on "inside the box and |v| < 6": the held-out accuracy (the last 5 000 of the 30 000
    rows; the first 25 000 train) of HipClsTrainer is not below the mean of ClsTrainer's over five seeds by more than
    their max - min, the reference loop's own seed noise.  Measured on an MI355X: see DESIGN section 21."""
    from vboc_amd.learn import ClsTrainer, HipClsTrainer
    F = _data(3, speed=6.0)
    train, held = F[:25000].contiguous(), F[25000:].contiguous()
    want = held[:, 7].to(torch.uint8)

    def accuracy(tr):
        assert tr.fit(train, it_max=300)["iterations"] == 300
        return float((tr.predict_labels(held[:, :6].contiguous())[0] == want).float().mean())

    ref = [accuracy(ClsTrainer(3, "cuda", seed=s, hidden=500, stop_val=0.0)) for s in range(5)]
    got = accuracy(HipClsTrainer(3, "cuda", seed=0, hidden=500, stop_val=0.0))
    print("ClsTrainer", ref, "HipClsTrainer", got, "majority class", float(max(want.float().mean(), 1 - want.float().mean())))
    assert got >= float(np.mean(ref)) - (max(ref) - min(ref)), (got, ref)
