"""The HJR main loop (pipeline.hjr_run) against a plain transcription of the reference's main block
(HJR/triplependulum_hjr.py:43-343, HJR/doublependulum_hjr.py, HJR/pendulum_hjr.py:40-190) written here with torch
and hjr.hjr_labels, on the same candidate arrays and the same minibatch indices, with the oracle's one-step OCP
(oracle/vboc_oracle_hjr.c); the three stop rules with a stub trainer; hjr_labels_arrays against hjr_labels; and on
the GPU the native trainer against the PyTorch trainer under the same sampler stream.
"""
import json
import math
import os
import random

import numpy as np
import pytest
import torch
from numpy.linalg import norm

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
V_MAX, V_MIN = 10.0, -10.0
Q_MAX, Q_MIN = np.pi / 4 + np.pi, -np.pi / 4 + np.pi


def oracle_factory(nq):
    class OracleHjr:
        def __init__(self, mean, std, params):
            self.mean, self.std = float(mean), float(std)
            self.W = [p.detach().cpu().numpy().astype(np.float64) for p in params]

        def compute_problems(self, X):
            r = oracle.hjr_solve_batch(nq, np.asarray(X, dtype=np.float64).reshape(-1, 2 * nq), self.W, self.mean,
                                       self.std)
            return (r["status"] == 0).astype(np.int64), r
    return OracleHjr


def reference_main_block(nq, X_test, B, hidden, it_max, max_iterations, seed, n_minibatch, loss_stop):
    """The main block of HJR/<sys>_hjr.py, statement by statement, with the candidate sets and the seeds injected;
    data_generation(v) over the set is hjr.hjr_labels (pinned to the reference's function by tests/test_hjr.py)."""
    from vboc_amd.hjr import hjr_labels
    from vboc_amd.ics import hjr_candidates
    from vboc_amd.learn import NeuralNetCLS
    device = torch.device("cpu")
    torch.manual_seed(seed)
    random.seed(seed)
    model = NeuralNetCLS(2 * nq, hidden, 2).to(device)
    criterion = torch.nn.BCEWithLogitsLoss()
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    beta = 0.95
    goes = (lambda it: it <= it_max) if nq == 1 else (lambda it: it < it_max)
    Xu_iter = hjr_candidates(nq, "init", B, 0, seed)
    Xu_test = hjr_candidates(nq, "test", B, 0, seed)
    Xu_iter_tensor = torch.from_numpy(Xu_iter.astype(np.float32)).to(device)
    mean, std = torch.mean(Xu_iter_tensor), torch.std(Xu_iter_tensor)
    X_iter = Xu_iter
    y_iter = np.array([[0, 1] if all(Xu_iter[n, i] >= Q_MIN and Xu_iter[n, i] <= Q_MAX for i in range(nq)) and
                       all(Xu_iter[n, i + nq] >= V_MIN and Xu_iter[n, i + nq] <= V_MAX for i in range(nq))
                       else [1, 0] for n in range(Xu_iter.shape[0])])

    def train():
        it, val = 0, 1
        while val > loss_stop and goes(it):
            ind = random.sample(range(X_iter.shape[0]), n_minibatch)
            X_iter_tensor = torch.from_numpy(X_iter[ind].astype(np.float32)).to(device)
            y_iter_tensor = torch.from_numpy(y_iter[ind].astype(np.float32)).to(device)
            X_iter_tensor = (X_iter_tensor - mean) / std
            outputs = model(X_iter_tensor)
            loss = criterion(outputs, y_iter_tensor)
            loss.backward()
            optimizer.step()
            optimizer.zero_grad()
            val = beta * val + (1 - beta) * loss.item()
            it += 1

    def positives():
        y_test_pred = np.argmax(model((torch.from_numpy(Xu_test.astype(np.float32)).to(device) - mean) / std)
                                .detach().cpu().numpy(), axis=1)
        return np.sum([1 for i in range(Xu_test.shape[0]) if y_test_pred[i] == 1]) / Xu_test.shape[0]

    def rmse_now():
        output_hjr_test = np.argmax(model((torch.Tensor(X_test).to(device) - mean) / std).cpu().detach().numpy(),
                                    axis=1)
        norm_error = np.empty((len(X_test),))
        for i in range(len(X_test)):
            vel_norm = norm([X_test[i][nq + j] for j in range(nq)])
            v = [X_test[i][nq + j] for j in range(nq)]
            sign = -1.0 if output_hjr_test[i] == 0 else 1.0
            out = output_hjr_test[i]
            while out == output_hjr_test[i] and norm(v) > 1e-2:
                if sign < 0:
                    v = [v[j] - 1e-2 * X_test[i][nq + j] / vel_norm for j in range(nq)]
                else:
                    v = [v[j] + 1e-2 * X_test[i][nq + j] / vel_norm for j in range(nq)]
                out = np.argmax(model((torch.Tensor([[X_test[i][j] for j in range(nq)] + v]).to(device) - mean) / std)
                                .cpu().detach().numpy(), axis=1)
            norm_error[i] = vel_norm - norm(v)
        return math.sqrt(np.sum(np.power(norm_error, 2)) / len(norm_error))

    train()
    pos_old = Xu_iter.shape[0]
    pos_new = positives()
    pos, rmse, kept = [pos_new], [], []
    if nq > 1:
        rmse.append(rmse_now())
    iterbreak = 0
    cap = {3: 120, 2: 150, 1: 100}[nq]
    while ((pos_new <= pos_old or iterbreak > 10) if nq > 1 else pos_new <= pos_old) and iterbreak < cap \
            and iterbreak < max_iterations:
        iterbreak = iterbreak + 1
        ocp = oracle_factory(nq)(mean.item(), std.item(), model.parameters())
        Xu_iter = hjr_candidates(nq, "iter", B, iterbreak, seed)
        with torch.no_grad():
            inp = (torch.from_numpy(Xu_iter.astype(np.float32)).to(device) - mean) / std
            y_pred = np.argmax(model(inp).detach().cpu().numpy(), axis=1)
        temp = hjr_labels(ocp, Xu_iter, y_pred)
        x, y = zip(*temp)
        X_iter, y_iter = np.array([i for i in x if i is not None]), np.array([i for i in y if i is not None])
        kept.append(temp)
        train()
        pos_old = pos_new
        pos_new = positives()
        pos.append(pos_new)
        if nq > 1:
            rmse.append(rmse_now())
    return dict(pos=np.array(pos), rmse=np.array(rmse), kept=kept, state=model.state_dict(), mean=mean, std=std,
                iterations=iterbreak)


def _heldout(nq, m=6, seed=3):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(m, nq))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.c_[rng.uniform(Q_MIN, Q_MAX, (m, nq)), d * rng.uniform(1.0, 9.0, (m, 1))]


@pytest.mark.parametrize("nq", [1, 2, 3])
def test_hjr_run_equals_the_reference_main_block(nq, tmp_path):
    from vboc_amd.pipeline import hjr_run
    B, hidden, it_max, seed, k = 512, 16, 40, 7, 64
    loss_stop = 1e-3 if nq == 1 else 5e-3
    X_test = _heldout(nq) if nq > 1 else None
    ref = reference_main_block(nq, X_test, B, hidden, it_max, 2, seed, k, loss_stop)
    r = hjr_run(nq, X_test, B=B, hidden=hidden, max_iterations=2, seed=seed, out_dir=str(tmp_path), device="cpu",
                ocp_factory=oracle_factory(nq), it_max=it_max + (1 if nq == 1 else 0), minibatch=k)
    assert r["iterations"] == ref["iterations"] == 2
    assert np.array_equal(r["pos"], ref["pos"])
    for (keep, lab1), temp in zip(r["kept"], ref["kept"]):
        assert [s is not None for s, _ in temp] == keep.tolist()
        assert [o == [0, 1] for _, o in temp] == (lab1.astype(bool) & keep).tolist()
        assert keep.sum() >= k
    sd = r["trainer"].model.state_dict()
    assert set(sd) == set(ref["state"])
    for key in sd:
        assert torch.equal(sd[key], ref["state"][key]), key
    assert float(r["mean"]) == float(ref["mean"]) and float(r["std"]) == float(ref["std"])
    if nq > 1:
        assert r["rmse"].shape == ref["rmse"].shape == (3,)
        assert np.abs(r["rmse"] - ref["rmse"]).max() <= 1e-12
        assert r["capped"] == 0 and len(r["times"]) == 3
    # artefacts in the reference's formats
    tag = f"{nq}dof_hjr"
    back = torch.load(os.path.join(tmp_path, f"model_{tag}"), weights_only=True)
    for key in sd:
        assert torch.equal(back[key], sd[key])
    assert float(torch.load(os.path.join(tmp_path, f"mean_{tag}"), weights_only=True)) == float(r["mean"])
    assert float(torch.load(os.path.join(tmp_path, f"std_{tag}"), weights_only=True)) == float(r["std"])
    if nq > 1:
        assert np.array_equal(np.load(os.path.join(tmp_path, f"rmse_{tag}.npy")), r["rmse"])
        assert np.array_equal(np.load(os.path.join(tmp_path, f"times_{tag}.npy")), r["times"])


class StubTrainer:
    """Scripted shares of the test set classified viable; no fit.  Calls of predict_labels: the first and then every
    second one classify the test set (the others the iteration's candidates, answered "not viable": no OCP)."""

    def __init__(self, nq, script, B):
        from vboc_amd.learn import NeuralNetCLS
        self.device = torch.device("cpu")
        self.model = NeuralNetCLS(2 * nq, 4, 2)
        self.script, self.B, self.calls = script, B, 0

    def fit(self, F, it_max):
        return dict(iterations=0, val=1.0, launched=0)

    def predict_labels(self, X):
        i, self.calls = self.calls, self.calls + 1
        cnt = int(round(self.script[i // 2] * self.B)) if i % 2 == 0 else 0
        return torch.zeros(X.shape[0], dtype=torch.uint8), cnt


class NoOcp:
    def __init__(self, *a):
        pass

    def compute_problems(self, X):
        raise AssertionError("no candidate is predicted viable")


def _stub_run(nq, script, max_iterations):
    from vboc_amd.pipeline import hjr_run
    B = 64
    return hjr_run(nq, None, B=B, max_iterations=max_iterations, device="cpu", ocp_factory=NoOcp,
                   trainer=StubTrainer(nq, script, B), it_max=1, minibatch=32)


def test_hjr_stop_rules():
    from vboc_amd.pipeline import hjr_continues
    # pos_old = B before the first iteration (a count against a fraction): the first iteration always runs
    rise3 = [0.5, 0.4, 0.3, 0.6] + [0.6] * 20
    assert _stub_run(3, rise3, 30)["iterations"] == 3            # pos_new > pos_old stops the triple before 11
    fall = [0.9 - 0.01 * i for i in range(12)]
    rise12 = fall + [0.95, 0.96, 0.97, 0.98, 0.99] + [1.0] * 20  # rises from iteration 12 on
    assert _stub_run(3, rise12, 15)["iterations"] == 15          # `iterbreak > 10` keeps it going
    assert _stub_run(2, rise12, 15)["iterations"] == 15
    assert _stub_run(1, rise12, 15)["iterations"] == 12          # the pendulum's rule has no such clause
    assert hjr_continues(3, 0.5, 0.4, 119) and not hjr_continues(3, 0.5, 0.4, 120)
    assert hjr_continues(2, 0.5, 0.4, 149) and not hjr_continues(2, 0.5, 0.4, 150)
    assert hjr_continues(2, 0.3, 0.4, 5, 3599.0) and not hjr_continues(2, 0.3, 0.4, 5, 3600.0)
    assert hjr_continues(3, 0.3, 0.4, 5, 21599.0) and not hjr_continues(3, 0.3, 0.4, 5, 21600.0)
    assert hjr_continues(1, 0.3, 0.4, 99) and not hjr_continues(1, 0.3, 0.4, 100)


def test_hjr_labels_arrays_equal_hjr_labels_on_the_golden_candidates():
    from vboc_amd.hjr import hjr_labels, hjr_labels_arrays
    g = json.load(open(os.path.join(HERE, "golden", "hjr_3.json")))
    z = np.load(os.path.join(HERE, "golden", "hjr_net_3.npz"))
    W = [z[k] for k in z.files]

    class OracleHjr:
        def compute_problems(self, X):
            r = oracle.hjr_solve_batch(3, X, W, g["mean"], g["std"])
            return (r["status"] == 0).astype(np.int64), r

    X, pred = np.array(g["X"]), np.array(g["y_pred"])
    assert X.shape[0] == 96
    out = hjr_labels(OracleHjr(), X, pred)
    keep, lab1 = hjr_labels_arrays(OracleHjr(), X, pred)
    assert keep.shape == lab1.shape == (96,)
    for i, (s, o) in enumerate(out):
        assert (s is not None) == bool(keep[i])
        if s is not None:
            assert o == ([0, 1] if lab1[i] else [1, 0])
    assert lab1.sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [3, 2])
def test_hjr_run_native_trainer_learns_like_the_torch_trainer(nq):
    """B = 4096, hidden 100, it_max 200, 2 iterations on the device OCP classes: the native fit against ClsTrainer on
    the GPU fed the native sampler's stream (a twin with the same seed).  pos within 1 % of B per iteration, rmse
    within 15 % (test_device_fit_learns_like_the_torch_trainer's bar for two trainers whose roundings part)."""
    from vboc_amd.learn import ClsTrainer, HipClsTrainer
    from vboc_amd.pipeline import hjr_run
    B, k, seed = 4096, 1024, 11
    X_test = _heldout(nq, m=200, seed=5)
    kw = dict(B=B, max_iterations=2, seed=seed, it_max=200, minibatch=k)
    a = hjr_run(nq, X_test, native=True, **kw)
    assert type(a["trainer"]) is HipClsTrainer
    twin = HipClsTrainer(nq, "cuda", seed=seed, minibatch=k)
    b = hjr_run(nq, X_test, trainer=ClsTrainer(nq, "cuda", seed=seed, minibatch=k, sampler=twin.sample), **kw)
    print("pos", a["pos"], b["pos"], "rmse", a["rmse"], b["rmse"], "capped", a["capped"], b["capped"],
          "fits", a["fits"], b["fits"])
    assert 1 <= a["iterations"] == b["iterations"] <= 2          # the stop rule may end the run after one
    assert np.abs(a["pos"] - b["pos"]).max() <= 0.01
    assert np.all(np.abs(a["rmse"] - b["rmse"]) <= 0.15 * np.abs(b["rmse"]))
    assert a["capped"] == 0 and b["capped"] == 0
