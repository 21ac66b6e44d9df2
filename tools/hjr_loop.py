"""Run the HJR loop on one GPU (pipeline.hjr_run: HJR/triplependulum_hjr.py:43-343 and its twins): held-out set
(`testing`), first fit, then labelling + refit + classification + RMSE march per iteration.  Prints one JSON line:
the wall time, its split into labelling / fit / classify / march, and the fit's step time.
--it-max caps the minibatch steps of each fit (the reference's cap is int(2e3 B / 4096) per fit).
--torch-eval runs the classification and the march on PyTorch as well (the kernels' comparator).
usage: python tools/hjr_loop.py --nq 3 --iters 2 --native --out /tmp/hjr
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vboc_amd.pipeline import HJR, hjr_run, make_test_set  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=3)
    ap.add_argument("--test", type=int, default=1000, help="held-out problems of the RMSE march (nq 2 and 3)")
    ap.add_argument("--B", type=int, default=None, help="candidates per set (default: the reference's)")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--it-max", type=int, default=None)
    ap.add_argument("--native", action=argparse.BooleanOptionalAction, default=False)
    ap.add_argument("--torch-eval", action="store_true",
                    help="classify and march on PyTorch too (the comparator of the eval and march kernels)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    X_test = None
    if a.nq > 1 and a.test:
        from vboc_amd.drivers import GpuBackend
        X_test, _ = make_test_set(a.nq, GpuBackend(a.nq), num_prob=a.test, first_id=10**8, out_dir=a.out)
    t = time.time()
    trainer = None
    if a.torch_eval:
        from vboc_amd.ics import SEED
        from vboc_amd.learn import ClsTrainer
        trainer = ClsTrainer(a.nq, a.device, minibatch=HJR[a.nq]["minibatch"], stop_val=HJR[a.nq]["loss_stop"],
                             seed=SEED % (1 << 31), native_eval=False)
    r = hjr_run(a.nq, X_test, B=a.B, max_iterations=a.iters, it_max=a.it_max, native=a.native, out_dir=a.out,
                device=a.device, trainer=trainer)
    wall = time.time() - t
    s = r["split"]
    steps = max(s["fit_steps"], 1)
    B = a.B or HJR[a.nq]["B"]
    n_cls = B * (1 + 2 * r["iterations"])
    print(json.dumps(dict(phase="hjr", nq=a.nq, native=a.native, trainer=type(r["trainer"]).__name__,
                          torch_eval=a.torch_eval, B=B,
                          iterations=r["iterations"], wall_s=round(wall, 2),
                          labelling_s=round(s["labelling"], 3), fit_s=round(s["fit"], 3),
                          classify_s=round(s["classify"], 3), march_s=round(s["march"], 3),
                          fit_steps=s["fit_steps"], fit_step_ms=round(1e3 * s["fit"] / steps, 4),
                          classify_rows_per_s=round(n_cls / max(s["classify"], 1e-9), 1),
                          march_rays=0 if X_test is None else int(X_test.shape[0]),
                          march_ms_each=round(1e3 * s["march"] / max(len(r["rmse"]), 1), 3),
                          fit_iterations=[f["iterations"] for f in r["fits"]], pos=[float(p) for p in r["pos"]],
                          rmse=[float(x) for x in r["rmse"]], capped=r["capped"],
                          times=[round(float(x), 3) for x in r["times"]])), flush=True)


if __name__ == "__main__":
    main()
