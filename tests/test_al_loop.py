"""The AL main loop (pipeline.al_run) against a plain transcription of the reference's main blocks
(AL/triplependulum_al.py:65-432, AL/doublependulum_al.py:64-420) written here with torch, scipy and al.nn_guess, on the
same pool, the same seeds and the oracle's labelling OCP (oracle/vboc_oracle_ft.c); the triple's AL march
(`norm([v0, v1])` in the outward loop) against its literal loop; the stop rule and the clamp of B with stubs; and on the
GPU the loop on the device library (learn.PoolScorer on csrc/pool.hip) with the real OCP classes.
"""
import math
import os
import random

import numpy as np
import pytest
import torch
from numpy.linalg import norm

import oracle
import oracle_chain as oc

HERE = os.path.dirname(os.path.abspath(__file__))


def _solve(nq):
    """oracle.al_solve_batch (bound with the triple's widths) or the same C function with the spec's nq."""
    return oracle.al_solve_batch if nq == 3 else oc.al_solve_batch


class OracleOcp:
    """al_run's `ocp` on the CPU oracle."""

    def __init__(self, nq):
        from vboc_amd.al import AlSpec
        self.spec = AlSpec(nq)
        self.nq = nq

    def labels(self, X):
        r = _solve(self.nq)(self.spec, np.asarray(X, dtype=np.float64))
        return r["label"], r["x"]

    def labels_guess(self, X, xg):
        r = _solve(self.nq)(self.spec, np.asarray(X, dtype=np.float64), x_guess=np.asarray(xg, dtype=np.float64))
        return r["label"], r["x"]


def _pool(nq, n, seed):
    """Rows uniform in the drivers' widened box; every second (triple) or fourth (double) row has its velocities scaled
    into |v_i| <= 1 (slow states: viable ones, so both labels occur)."""
    from vboc_amd.al import AlSpec, unlabeled_states
    X = unlabeled_states(AlSpec(nq), n, np.random.default_rng(seed))
    X[::{3: 2, 2: 4}[nq], nq:] *= 1.0 / 11.0
    return X


def _heldout(nq, m=6, seed=3):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(m, nq))
    d /= np.linalg.norm(d, axis=1)[:, None]
    q_min, q_max = 3 * np.pi / 4, 5 * np.pi / 4
    return np.c_[rng.uniform(q_min, q_max, (m, nq)), d * rng.uniform(1.0, 9.0, (m, 1))]


def reference_main_block(nq, pool, X_test, N_init, B, hidden_size, n_minibatch, it_max, max_iterations, seed):
    """The main block of AL/triplependulum_al.py (nq 3) / AL/doublependulum_al.py (nq 2), statement by statement, with
    the pool and the seeds injected and ocp.compute_problem / compute_problem_nnguess on the oracle."""
    from scipy.stats import entropy
    from torch.utils.data import DataLoader
    from vboc_amd.al import AlSpec, nn_guess
    from vboc_amd.learn import NeuralNetCLS
    spec = AlSpec(nq)
    solve = _solve(nq)
    ocp_dim, ocp_N = 2 * nq, spec.N
    v_max, v_min, q_max, q_min = spec.dthetamax, -spec.dthetamax, spec.thetamax, spec.thetamin
    device = torch.device("cpu")
    etp_stop, loss_stop, beta = 0.1, 0.1, 0.95
    n_minibatch_model = pow(2, 15)
    torch.manual_seed(seed)
    random.seed(seed)
    model = NeuralNetCLS(ocp_dim, hidden_size, 2).to(device)
    model_guess = NeuralNetCLS(ocp_dim, hidden_size, ocp_dim * ocp_N).to(device)
    criterion = torch.nn.BCEWithLogitsLoss()
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    criterion_guess = torch.nn.MSELoss()
    optimizer_guess = torch.optim.Adam(model_guess.parameters(), lr=1e-3)

    def outside(q0, v0):
        return any(q0[j] < q_min or q0[j] > q_max or v0[j] < v_min or v0[j] > v_max for j in range(nq))

    def result(s0, r):
        res = int(r["label"][0])
        if res == 1:
            sim = np.reshape(r["x"][0], (ocp_N + 1) * ocp_dim,).tolist()
            return [*s0, 0, 1], sim
        elif res == 0:
            return [*s0, 1, 0], None

    def testing(s0):
        q0, v0 = s0[:nq], s0[nq:]
        if outside(q0, v0):
            return [*s0, 1, 0], None
        return result(s0, solve(spec, np.array(s0)[None], nthreads=1))

    def testing_guess(s0):
        q0, v0 = s0[:nq], s0[nq:]
        if outside(q0, v0):
            return [*s0, 1, 0], None
        xg = nn_guess(ocp_N, q0, v0, model_guess, mean, std)
        return result(s0, solve(spec, np.array(s0)[None], x_guess=xg[None], nthreads=1))

    Xu_iter = np.asarray(pool).tolist()
    Xu_iter_tensor = torch.Tensor(Xu_iter).to(device)
    mean, std = torch.mean(Xu_iter_tensor).to(device), torch.std(Xu_iter_tensor).to(device)
    temp = list(map(testing, Xu_iter[:N_init]))
    X_iter, X_traj = zip(*temp)
    X_traj = [i for i in X_traj if i is not None]
    del Xu_iter[:N_init]
    label_counts = [(sum(r[-1] for r in X_iter), len(X_iter))]

    def train_model(ind_fn):
        it, val = 0, 1
        while val > loss_stop and it <= it_max:
            ind = ind_fn()
            X_iter_tensor = torch.Tensor([X_iter[i][:ocp_dim] for i in ind]).to(device)
            y_iter_tensor = torch.Tensor([X_iter[i][ocp_dim:] for i in ind]).to(device)
            X_iter_tensor = (X_iter_tensor - mean) / std
            for param in model.parameters():
                param.grad = None
            outputs = model(X_iter_tensor)
            loss = criterion(outputs, y_iter_tensor)
            loss.backward()
            optimizer.step()
            val = beta * val + (1 - beta) * loss.item()
            it += 1

    def train_guess(qt):
        it, val = 0, 1
        while val > loss_stop and it <= it_max:
            if len(X_traj) < qt:
                qt = len(X_traj)
            ind = random.sample(range(len(X_traj)), qt)
            X_iter_tensor = torch.Tensor([X_traj[i][:ocp_dim] for i in ind]).to(device)
            y_iter_tensor = torch.Tensor([X_traj[i][ocp_dim:] for i in ind]).to(device)
            X_iter_tensor = (X_iter_tensor - mean) / std
            y_iter_tensor = (y_iter_tensor - mean) / std
            outputs = model_guess(X_iter_tensor)
            loss = criterion_guess(outputs, y_iter_tensor)
            loss.backward()
            optimizer_guess.step()
            optimizer_guess.zero_grad()
            val = beta * val + (1 - beta) * loss.item()
            it += 1

    def cls_of(row):
        return np.argmax(model((torch.Tensor([row]).to(device) - mean) / std).cpu().detach().numpy(), axis=1)

    def rmse_now():
        output_al_test = np.argmax(model((torch.Tensor(X_test).to(device) - mean) / std).cpu().detach().numpy(), axis=1)
        norm_error_al = np.empty((len(X_test),))
        for i in range(len(X_test)):
            vt = [X_test[i][nq + j] for j in range(nq)]
            vel_norm = norm(vt)
            v = list(vt)
            if output_al_test[i] == 0:
                out = 0
                while out == 0 and norm(v) > 1e-2:
                    v = [v[j] - 1e-2 * vt[j] / vel_norm for j in range(nq)]
                    out = cls_of([X_test[i][j] for j in range(nq)] + v)
            else:
                out = 1
                while out == 1 and norm([v[0], v[1]]) > 1e-2:       # both drivers: two components
                    v = [v[j] + 1e-2 * vt[j] / vel_norm for j in range(nq)]
                    out = cls_of([X_test[i][j] for j in range(nq)] + v)
                    assert norm(v) < 100.0, "the reference's outward march has no bound: an input condition"
            norm_error_al[i] = vel_norm - norm(v)
        return math.sqrt(np.sum(np.power(norm_error_al, 2)) / len(norm_error_al))

    train_model(lambda: random.sample(range(len(X_iter)), n_minibatch))
    qt = n_minibatch
    train_guess(qt)
    rmse = np.array([rmse_now()])
    k, etpmax = 0, 1
    sigmoid = torch.nn.Sigmoid()
    queries, etps = [], []
    while not (etpmax < etp_stop or len(Xu_iter) == 0) and k < max_iterations:
        if len(Xu_iter) < B:
            B = len(Xu_iter)
        etp = np.empty((len(Xu_iter),))
        with torch.no_grad():
            Xu_iter_tensor = torch.Tensor(Xu_iter).to(device)
            Xu_iter_tensor = (Xu_iter_tensor - mean) / std
            my_dataloader = DataLoader(Xu_iter_tensor, batch_size=n_minibatch_model, shuffle=False)
            for (idx, batch) in enumerate(my_dataloader):
                if n_minibatch_model * (idx + 1) > len(Xu_iter):
                    prob_xu = sigmoid(model(batch)).cpu()
                    etp[n_minibatch_model * idx:len(Xu_iter)] = entropy(prob_xu, axis=1)
                else:
                    prob_xu = sigmoid(model(batch)).cpu()
                    etp[n_minibatch_model * idx:n_minibatch_model * (idx + 1)] = entropy(prob_xu, axis=1)
        maxindex = np.argpartition(etp, -B)[-B:].tolist()
        maxindex.sort(reverse=True)
        etpmax = max(etp[maxindex])
        k += 1
        elems = [None] * B
        for i in range(B):
            elems[i] = Xu_iter[maxindex[i]]
            del Xu_iter[maxindex[i]]
        temp = list(map(testing_guess, elems))
        tmp1, tmp2 = zip(*temp)
        label_counts.append((sum(r[-1] for r in tmp1), len(tmp1)))
        queries.append(maxindex)
        etps.append(etpmax)
        if nq == 3:
            qt = B if len(X_traj) > B else len(X_traj)
            qi = B if len(X_iter) > B else len(X_iter)
            tp = [i for i in tmp2 if i is not None]
            X_traj = X_traj[qt:] + tp
            X_iter = X_iter[qi:] + tmp1
            train_model(lambda: random.sample(range(len(X_iter)), n_minibatch))
        else:
            X_iter = X_iter + tmp1
            tp = [i for i in tmp2 if i is not None]
            qn = n_minibatch if len(X_traj) > n_minibatch else len(X_traj)
            ind = random.sample(range(len(X_traj)), qn)
            tkeep = [i for i in X_traj if i in ind]
            X_traj = tkeep + tp
            train_model(lambda: random.sample(range(len(X_iter) - B), int(n_minibatch / 2)) +
                        random.sample(range(len(X_iter) - B, len(X_iter)), int(n_minibatch / 2)))
            qt = n_minibatch
        train_guess(qt)
        rmse = np.append(rmse, [rmse_now()])
    return dict(rmse=rmse, queries=queries, etpmax=etps, state=model.state_dict(), state_guess=model_guess.state_dict(),
                mean=mean, std=std, X_iter=np.asarray(X_iter), label_counts=label_counts, pool=np.asarray(Xu_iter))


@pytest.mark.parametrize("nq", [3, 2])
def test_al_run_equals_the_reference_main_block(nq, tmp_path):
    from vboc_amd.pipeline import al_run
    # A second input condition: the reference's outward march has no bound, and a classifier of 21 steps can label a
    # whole ray 1.  The seeds are ones at which every march of the transcription ends (it asserts |v| < 100).
    n, N_init, hidden, k, it_max, seed = 1024, 128, 16, 64, 20, {3: 1, 2: 2}[nq]
    pool = _pool(nq, n, seed=20 + nq)
    X_test = _heldout(nq)
    ref = reference_main_block(nq, pool, X_test, N_init, N_init, hidden, k, it_max, 2, seed)
    # the input condition: both labels in the initial set and in each query batch
    assert len(ref["label_counts"]) == 3
    for ones, total in ref["label_counts"]:
        assert 0 < ones < total == N_init, ref["label_counts"]
    r = al_run(nq, X_test, pool=pool, ocp=OracleOcp(nq), B=N_init, N_init=N_init, hidden=hidden, minibatch=k,
               it_max=it_max, max_iterations=2, seed=seed, device="cpu", out_dir=str(tmp_path))
    assert r["iterations"] == 2 and r["dropped"] == 0 and r["labels"][2] == 0
    assert float(r["mean"]) == float(ref["mean"]) and float(r["std"]) == float(ref["std"])
    for got, want in zip(r["queries"], ref["queries"]):
        assert got.tolist() == want
    assert [float(e) for e in r["etpmax"]] == [float(e) for e in ref["etpmax"]]
    for sd, want in ((r["trainer"].model.state_dict(), ref["state"]),
                     (r["guess_trainer"].model.state_dict(), ref["state_guess"])):
        assert set(sd) == set(want)
        for key in sd:
            assert torch.equal(sd[key], want[key]), key
    assert np.array_equal(r["X_iter"], ref["X_iter"])
    assert np.array_equal(np.asarray(r["pool"]), ref["pool"])
    assert r["rmse"].shape == ref["rmse"].shape == (3,) and len(r["times"]) == 3
    assert np.abs(r["rmse"] - ref["rmse"]).max() <= 1e-12
    assert set(r["split"]) >= {"entropy", "select", "guess", "labelling", "fit_cls", "fit_guess", "march"}
    # artefacts in the reference's formats
    sd = r["trainer"].model.state_dict()
    back = torch.load(os.path.join(tmp_path, f"model_{nq}dof"), weights_only=True)
    for key in sd:
        assert torch.equal(back[key], sd[key])
    assert float(torch.load(os.path.join(tmp_path, f"mean_{nq}dof_al"), weights_only=True)) == float(r["mean"])
    assert float(torch.load(os.path.join(tmp_path, f"std_{nq}dof_al"), weights_only=True)) == float(r["std"])
    assert np.array_equal(np.load(os.path.join(tmp_path, f"rmse_{nq}dof_al.npy")), r["rmse"])
    assert np.array_equal(np.load(os.path.join(tmp_path, f"times_{nq}dof_al.npy")), r["times"])
    assert np.array_equal(np.load(os.path.join(tmp_path, f"data_{nq}dof_al.npy")), r["X_iter"])


def test_march_outward_dims_equals_the_triples_literal_loop_on_8_rays():
    """learn.march_reference(outward_dims=2) against a literal transcription of AL/triplependulum_al.py:206-227 (one
    ray at a time, one point per classifier call), and the default against the same loop with the full norm in both
    branches (HJR/triplependulum_hjr.py:152-174, what march_reference restated before).  The classifier is a small
    torch network evaluated in float64 on the float32 cast of each point, so that a batched and a single-row forward
    agree.  Two rays start at label 1 with |(v0, v1)| <= 1e-2 and v2 large: the AL loop takes no step on them."""
    from vboc_amd.learn import ClsTrainer, march_reference
    nq = 3
    rng = np.random.default_rng(1)
    q_min, q_max = 3 * np.pi / 4, 5 * np.pi / 4
    Xf = np.c_[rng.uniform(q_min, q_max, (20000, nq)), rng.uniform(-11, 11, (20000, nq))].astype(np.float32)
    Xt = torch.from_numpy(Xf)
    mean_t, std_t = torch.mean(Xt), torch.std(Xt)
    inside = np.linalg.norm(Xf[:, nq:], axis=1) < 9.0
    F = torch.cat([(Xt - mean_t) / std_t, torch.from_numpy(np.c_[~inside, inside].astype(np.float32))], dim=1)
    tr = ClsTrainer(nq, "cpu", hidden=16, minibatch=256, lr=1e-2, stop_val=0.0, seed=3)
    tr.fit(F, it_max=800)
    model = tr.model.double()
    mean, std = mean_t.double(), std_t.double()

    @torch.no_grad()
    def classify(P):
        out = model((torch.from_numpy(np.asarray(P, dtype=np.float32)).double() - mean) / std)
        return np.argmax(out.numpy(), axis=1)

    d = rng.normal(size=(6, nq))
    d /= np.linalg.norm(d, axis=1)[:, None]
    X_test = np.c_[rng.uniform(q_min, q_max, (8, nq)),
                   np.vstack([d * np.array([1.0, 2.5, 4.0, 10.5, 11.0, 12.0])[:, None],
                              [0.004, -0.003, 2.0], [0.0, 0.006, -1.5]])]
    start = classify(X_test)
    assert 2 <= start[:6].sum() <= 4 and start[6] == 1 and start[7] == 1, start

    def literal(al):
        output_al_test = classify(X_test)
        norm_error_al, count = np.empty((len(X_test),)), np.zeros(len(X_test), dtype=int)
        for i in range(len(X_test)):
            vel_norm = norm([X_test[i][3], X_test[i][4], X_test[i][5]])
            v0, v1, v2 = X_test[i][3], X_test[i][4], X_test[i][5]
            if output_al_test[i] == 0:
                out = 0
                while out == 0 and norm([v0, v1, v2]) > 1e-2:
                    v0 = v0 - 1e-2 * X_test[i][3] / vel_norm
                    v1 = v1 - 1e-2 * X_test[i][4] / vel_norm
                    v2 = v2 - 1e-2 * X_test[i][5] / vel_norm
                    out = classify([[X_test[i][0], X_test[i][1], X_test[i][2], v0, v1, v2]])
                    count[i] += 1
            else:
                out = 1
                while out == 1 and (norm([v0, v1]) if al else norm([v0, v1, v2])) > 1e-2:
                    v0 = v0 + 1e-2 * X_test[i][3] / vel_norm
                    v1 = v1 + 1e-2 * X_test[i][4] / vel_norm
                    v2 = v2 + 1e-2 * X_test[i][5] / vel_norm
                    out = classify([[X_test[i][0], X_test[i][1], X_test[i][2], v0, v1, v2]])
                    count[i] += 1
                    assert count[i] < 5000
            norm_error_al[i] = vel_norm - norm([v0, v1, v2])
        return norm_error_al, count, output_al_test

    for al, kw in ((True, dict(outward_dims=2)), (False, dict())):
        want, count, lab = literal(al)
        err, steps, flags = march_reference(classify, X_test, float(mean), float(std), **kw)
        assert np.array_equal(steps, count) and np.array_equal(flags, lab.astype(np.uint8)), (al, steps, count)
        assert np.abs(err - want).max() <= 1e-12
        assert count[:6].min() > 0
        if al:
            assert count[6] == 0 and count[7] == 0 and err[6] == 0.0
        else:
            assert count[6] > 100 and count[7] > 100


class StubScorer:
    """Scripted etpmax values; the scores rise with the row index, so the query is the pool's tail."""

    def __init__(self, nq, script):
        self.nq, self.script, self.k = nq, script, 0

    def to_pool(self, X):
        return np.ascontiguousarray(X, dtype=np.float64)

    def entropy(self, X, mean, std):
        return np.arange(X.shape[0], dtype=np.float64)

    def select(self, etp, X, B):
        idx = np.arange(X.shape[0] - 1, X.shape[0] - 1 - B, -1)
        e, self.k = self.script[min(self.k, len(self.script) - 1)], self.k + 1
        return dict(idx=idx, scores=etp[idx], X_sel=X[idx], X_rest=np.delete(X, idx, 0), etpmax=e)

    def guess(self, X0, N, mean, std):
        return np.zeros((X0.shape[0], N + 1, 2 * self.nq))


class StubOcp:
    """Every second state viable, with a trajectory of zeros."""

    def __init__(self, nq):
        from vboc_amd.al import AlSpec
        self.spec = AlSpec(nq)

    def labels(self, X):
        return np.arange(X.shape[0]) % 2, np.zeros((X.shape[0], self.spec.N + 1, self.spec.nx))

    def labels_guess(self, X, xg):
        assert xg.shape == (X.shape[0], self.spec.N + 1, self.spec.nx)
        return self.labels(X)


def _stub_run(nq, script, n=100, **kw):
    from vboc_amd.al import AlSpec
    from vboc_amd.pipeline import al_run
    rng = np.random.default_rng(0)
    s = AlSpec(nq)
    pool = np.c_[rng.uniform(s.thetamin, s.thetamax, (n, nq)), rng.uniform(-9, 9, (n, nq))]
    a = dict(pool=pool, ocp=StubOcp(nq), B=32, N_init=32, hidden=4, minibatch=8, it_max=0, device="cpu",
             scorer=StubScorer(nq, script), seed=1)
    a.update(kw)
    return al_run(nq, None, **a)


@pytest.mark.parametrize("nq", [3, 2])
def test_al_stop_rule_and_the_clamp_of_B(nq):
    from vboc_amd.pipeline import AL, al_continues
    # etpmax < etp_stop ends the loop at the next test of the condition
    r = _stub_run(nq, [0.5, 0.05, 0.5], n=1000)
    assert r["iterations"] == 2 and r["etpmax"].tolist() == [0.5, 0.05] and r["pool_rows"] == 1000 - 32 - 64
    # the pool runs out: B is clamped to the remainder (68 rows after the initial set: 32, 32, 4)
    r = _stub_run(nq, [0.5])
    assert r["iterations"] == 3 and [len(q) for q in r["queries"]] == [32, 32, 4] and r["pool_rows"] == 0
    assert r["labels"][0] + r["labels"][1] == 100 and r["labels"][2] == 0 and len(r["times"]) == 4
    # the clock
    assert _stub_run(nq, [0.5], max_time=0.0)["iterations"] == 0
    assert _stub_run(nq, [0.5], max_iterations=1)["iterations"] == 1
    t = AL[nq]["max_time"]
    assert t == {3: 21600.0, 2: 3450.0}[nq]
    assert al_continues(1, 10, t - 1.0, t) and not al_continues(1, 10, t, t)
    assert al_continues(0.1, 10, 0.0, t) and not al_continues(0.0999, 10, 0.0, t) and not al_continues(1, 0, 0.0, t)
    assert (AL[3]["B"], AL[3]["N_init"], AL[3]["hidden"], AL[3]["gridp"]) == (6 ** 6, 6 ** 6, 500, 15)
    assert (AL[2]["B"], AL[2]["N_init"], AL[2]["hidden"], AL[2]["gridp"]) == (10 ** 4, 10 ** 4, 300, 60)


def test_al_run_drops_and_counts_label_2():
    """The one deviation from the reference: a state labelled 2 leaves the labelled set and is counted."""
    class Ocp2(StubOcp):
        def labels(self, X):
            lab, x = super().labels(X)
            lab[:3] = 2
            return lab, x
    r = _stub_run(3, [0.5], n=64, ocp=Ocp2(3), max_iterations=1)
    assert r["dropped"] == 6 and r["labels"][2] == 6
    assert r["X_iter"].shape == (32 - 3, 8) and set(np.unique(r["X_iter"][:, 6:])) <= {0.0, 1.0}


# ----------------------------------------------------------------------------------------------------------------
# on the GPU: the device scorer inside the loop, on the real OCP classes
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nq", [3, 2])
def test_al_run_on_the_device_scorer(nq):
    """pool 4096, N_init = B = 256, hidden 100, minibatch 64, it_max 20, two iterations on OCP<sys>INIT.  The queried
    rows satisfy test_pool_device's ranking condition (its docstring derives eps) against the float64 forward of the
    classifier as it stood at that iteration; the labels equal a second, direct compute_problem_guess_batch on the
    same states and the scorer's guesses."""
    from test_pool_device import entropy64, ranking_ok
    from vboc_amd import al as al_mod
    from vboc_amd.learn import NeuralNetCLS, PoolScorer
    from vboc_amd.pipeline import al_run
    n, B = 4096, 256
    pool = _pool(nq, n, seed=40 + nq)
    X_test = _heldout(nq, m=50, seed=5)
    r = al_run(nq, X_test, pool=pool, B=B, N_init=B, hidden=100, minibatch=64, it_max=20, max_iterations=2, seed=3,
               device="cuda")
    assert type(r["scorer"]) is PoolScorer and r["scorer"].native
    assert r["iterations"] == 2 and r["pool_rows"] == n - 3 * B and len(r["rmse"]) == 3
    left = r["pool"].cpu().numpy()
    assert left.shape == (n - 3 * B, 2 * nq)
    cur = pool[B:]
    mean, std = float(r["mean"]), float(r["std"])
    ocp = {3: al_mod.OCPtriplependulumINIT, 2: al_mod.OCPdoublependulumINIT}[nq]()
    for it in range(2):
        idx = r["queries"][it]
        assert idx.shape == (B,) and np.all(np.diff(idx) < 0)
        W = [r["cls_states"][it][k].numpy().astype(np.float64) for k in r["cls_states"][it]]
        e64, eps = entropy64(W, cur, mean, std)
        ranking_ok(e64, eps, idx, B)
        assert np.array_equal(r["scores"][it].max(), np.float32(r["etpmax"][it]))
        b = r["batches"][it]
        assert np.array_equal(b["S"], cur[idx])
        # the labels again, directly: the guess network as it stood, the scorer's guesses, the class's own batch call
        g = NeuralNetCLS(2 * nq, 100, 2 * nq * ocp.N).cuda()
        g.load_state_dict(r["guess_states"][it])
        sc = PoolScorer(nq, r["trainer"].model, g, "cuda")
        x0 = b["S"][b["inb"]]
        xg = sc.guess(x0, ocp.N, mean, std).cpu().numpy()
        again = ocp.compute_problem_guess_batch(x0, xg)["label"]
        assert np.array_equal(again, b["label"][b["inb"]])
        assert np.all(b["label"][~b["inb"]] == 0)
        cur = np.delete(cur, idx, 0)
    assert np.array_equal(left, cur)
    q = {tuple(row) for it in range(2) for row in r["batches"][it]["S"]}
    assert not any(tuple(row) in q for row in left)
