"""Run the AL loop on one GPU (pipeline.al_run: AL/triplependulum_al.py:65-432 and the double's twin) at the
reference's shapes: the initial labels and fits, then per iteration the pool's entropy, the top-B selection, the guess
trajectories, the labelling OCP, both refits and the RMSE march.  Prints one JSON line and, with --out, writes it to
profiles/al_loop_<triple|double>_<device|torch>.json: the wall time, its split, the per-call times of the three pool
operations, the pool size and the entropy pass's rate against the FP32 matrix peak.
--fit-steps caps the minibatch steps of each fit (the reference's cap is int(1e2 B / 4096) + 1 per fit).
--torch runs the pool operations on the torch / NumPy path of the same commit on the same GPU (the comparator: the
reference's arithmetic).
--march device | torch picks the RMSE march: the scorer's kernel (vboc_pool_boundary) or march_reference on the torch
module (the comparator); auto is al_run's default.  With it the file name gains _march_<device|torch>.
--native-fit fits the classifier on the device library (al_run(native_fit=True)); the file name gains _native_fit.
usage: python tools/al_loop.py --nq 3 --iters 1 --fit-steps 200 --out profiles
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from vboc_amd.pipeline import AL, al_run  # noqa: E402

FP32_MATRIX_PEAK = 157e12       # MI355X, flop/s (guide figure)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=3)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--fit-steps", type=int, default=200)
    ap.add_argument("--test", type=int, default=100, help="held-out rays of the RMSE march (0: no march)")
    ap.add_argument("--torch", action="store_true", help="pool operations on the torch / NumPy path")
    ap.add_argument("--march", choices=("auto", "device", "torch"), default="auto", help="the RMSE march's path")
    ap.add_argument("--native-fit", action="store_true", help="the classifier's fits on csrc/cls.hip")
    ap.add_argument("--B", type=int, default=None)
    ap.add_argument("--pool", type=int, default=None, help="pool rows (default: the reference's gridp ** (2 nq))")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    c = AL[a.nq]
    rng = np.random.default_rng(1)
    X_test = None
    if a.test:
        d = rng.normal(size=(a.test, a.nq))
        d /= np.linalg.norm(d, axis=1)[:, None]
        X_test = np.c_[rng.uniform(3 * np.pi / 4, 5 * np.pi / 4, (a.test, a.nq)), d * rng.uniform(1.0, 9.0, (a.test, 1))]
    pool = None
    if a.pool:
        from vboc_amd.al import AlSpec, unlabeled_states
        pool = unlabeled_states(AlSpec(a.nq), a.pool, rng)
    t = time.time()
    r = al_run(a.nq, X_test, pool=pool, B=a.B, N_init=a.B, max_iterations=a.iters, device=a.device,
               native=not a.torch, fit_steps=a.fit_steps,
               device_march={"auto": None, "device": True, "torch": False}[a.march], native_fit=a.native_fit)
    wall = time.time() - t
    s, calls = r["split"], r["scorer"].calls
    B = a.B or c["B"]
    n0 = (a.pool or c["gridp"] ** (2 * a.nq)) - B
    hidden = c["hidden"]
    ent = calls["entropy"]
    flop = 2.0 * n0 * (2 * a.nq * hidden + hidden * hidden + 2 * hidden)     # the first pass's rows, real widths
    out = dict(phase="al", nq=a.nq, scorer="torch" if a.torch else "device", B=B, pool_rows_first_pass=n0,
               hidden=hidden, iterations=r["iterations"], fit_steps_cap=a.fit_steps, wall_s=round(wall, 2),
               native_fit=r["native_fit"], fit_cls_s=round(s["fit_cls"], 4), fit_cls_steps=s["fit_cls_steps"],
               fit_cls_ms_per_step=round(1e3 * s["fit_cls"] / max(s["fit_cls_steps"], 1), 4),
               split={k: (round(v, 4) if isinstance(v, float) else v) for k, v in s.items()},
               entropy_call_s=[round(x, 5) for x in ent], select_call_s=[round(x, 5) for x in calls["select"]],
               guess_call_s=[round(x, 5) for x in calls["guess"]],
               march="device" if r["device_march"] else "torch", test=a.test,
               march_call_s=[round(x, 5) for x in r["march_s"]], capped=r["capped"],
               entropy_flop=flop, entropy_tflops=round(flop / max(ent[0], 1e-12) / 1e12, 3) if ent else None,
               entropy_share_of_fp32_matrix_peak=round(flop / max(ent[0], 1e-12) / FP32_MATRIX_PEAK, 4) if ent else None,
               labels=r["labels"], dropped=r["dropped"], etpmax=[float(e) for e in r["etpmax"]],
               rmse=[float(x) for x in r["rmse"]], times=[round(float(x), 3) for x in r["times"]],
               pool_rows_left=r["pool_rows"])
    print(json.dumps(out), flush=True)
    print(f"fit_cls {out['fit_cls_s']} s, {out['fit_cls_steps']} steps, {out['fit_cls_ms_per_step']} ms per step "
          f"({'native' if r['native_fit'] else 'torch'})", file=sys.stderr, flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        name = f"al_loop_{'triple' if a.nq == 3 else 'double'}_{'torch' if a.torch else 'device'}" \
               f"{'' if a.march == 'auto' else '_march_' + a.march}{'_native_fit' if a.native_fit else ''}.json"
        with open(os.path.join(a.out, name), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
