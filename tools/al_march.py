"""Time AL's RMSE march alone on one GPU, both ways in one process: learn.PoolScorer.boundary on the device kernel
(vboc_pool_boundary) against the torch path of the same scorer class (march_reference on the module), alternating, on
the same classifier and the same held-out rays.  The classifier is NeuralNetCLS(2nq, hidden, 2) after --fit-steps torch
steps on ball labels (|v| < 6), so that rays march inward and outward to a boundary inside the velocity box; the rays
are tools/al_loop.py's.  Prints one JSON line (seconds per call: every sample, min, median, max) and, with --out, writes
it to <out>/al_march_<triple|double>.json.
usage: python tools/al_march.py --nq 3 --test 1000 --repeats 10 --out profiles
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vboc_amd.learn import ClsTrainer, PoolScorer  # noqa: E402
from vboc_amd.pipeline import AL  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=3)
    ap.add_argument("--test", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--fit-steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nq, hidden = a.nq, AL[a.nq]["hidden"]
    rng = np.random.default_rng(1)
    d = rng.normal(size=(a.test, nq))
    d /= np.linalg.norm(d, axis=1)[:, None]
    q_min, q_max = 3 * np.pi / 4, 5 * np.pi / 4
    X_test = np.c_[rng.uniform(q_min, q_max, (a.test, nq)), d * rng.uniform(1.0, 9.0, (a.test, 1))]
    X = np.c_[rng.uniform(q_min, q_max, (30000, nq)), rng.uniform(-8.0, 8.0, (30000, nq))]
    Xf = torch.from_numpy(X.astype(np.float32))
    mean, std = torch.mean(Xf), torch.std(Xf)
    inside = np.linalg.norm(X[:, nq:], axis=1) < 6.0
    F = torch.cat([(Xf - mean) / std, torch.from_numpy(np.c_[~inside, inside].astype(np.float32))], dim=1)
    tr = ClsTrainer(nq, "cuda", hidden=hidden, minibatch=1024, lr=3e-3, stop_val=0.0, seed=1, native_eval=False)
    tr.fit(F, it_max=a.fit_steps)
    od = 2 if nq == 3 else None
    dev = PoolScorer(nq, tr.model, None, "cuda")
    ref = PoolScorer(nq, tr.model, None, "cuda", native=False)
    Xd = dev.to_pool(X_test)
    mean, std = float(mean), float(std)
    bd = dev.boundary(Xd, mean, std, outward_dims=od)        # warm-up: both paths once, not counted
    br = ref.boundary(X_test, mean, std, outward_dims=od)
    dev.calls["boundary"].clear()
    ref.calls["boundary"].clear()
    for _ in range(a.repeats):
        dev.boundary(Xd, mean, std, outward_dims=od)
        ref.boundary(X_test, mean, std, outward_dims=od)

    def stats(x):
        return dict(samples=[round(v, 6) for v in x], min=round(min(x), 6), median=round(float(np.median(x)), 6),
                    max=round(max(x), 6))
    out = dict(phase="al_march", nq=nq, hidden=hidden, test=a.test, repeats=a.repeats, fit_steps=a.fit_steps,
               device_s=stats(dev.calls["boundary"]), torch_s=stats(ref.calls["boundary"]),
               steps_device=dict(min=int(bd["steps"].min()), max=int(bd["steps"].max()), sum=int(bd["steps"].sum())),
               steps_torch_sum=int(br["steps"].sum()), rays_with_equal_steps=int((bd["steps"] == br["steps"]).sum()),
               capped=[bd["capped"], br["capped"]], rmse=[bd["rmse"], br["rmse"]],
               label_1=int((bd["flags"] & 1).sum()))
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, f"al_march_{'triple' if nq == 3 else 'double'}.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
