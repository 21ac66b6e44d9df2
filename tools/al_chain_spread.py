"""The oracle's own rounding spread on the AL labelling cases of tests/test_al_chains.py (the double pendulum at
N in {1, 3, 65, 100}, the pendulum at N in {1, 100}; 96 states each, the short-horizon ones filtered by the LP as the
test does).  CPU only.  The method is tools/trunc_spread.py's: the oracle built with its four compiler-flag sets
(VARIANTS there), every build run in a child process on every case, and per case written to
tests/golden/al_chain_spread.json:

  * n: the states of the case;
  * labels_differ / qp_iter_differ: the states on which some build's label / QP iteration count is not the committed
    build's, and of the former those where no build is at the iteration cap (not_at_cap);
  * spread_x / spread_u: over the states every build labels 1, the largest |dx| / |du| against the committed build.

An infeasible QP has no solution for the interior point to converge to: its iterates grow until a factorisation fails
or - at N = 1 and N = 3 - the stop test passes on a point that is none, and WHICH of the two
happens, and at which iteration, is decided by rounding.  The fixture shows how often the oracle parts from itself there;
tests/test_al_chains.py takes its short-horizon bars on the discrete quantities from it.

usage: python tools/al_chain_spread.py [--out FILE]
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trunc_spread as ts  # noqa: E402

ROOT = ts.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "al_chain_spread.json")


def _cases():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    import test_al_chains as t
    return t


def _child(out):
    t = _cases()
    import oracle
    import oracle_chain as oc
    assert os.environ.get("VBOC_ORACLE_LIB") and oracle.LIB == os.environ["VBOC_ORACLE_LIB"]
    states = np.load(os.environ["VBOC_AL_STATES"])
    save = {}
    for nq, N, _ in t.CASES:
        r = oc.al_solve_batch(t.al_spec(nq, N), states[f"{nq}|{N}"])
        for k, v in r.items():
            save[f"{nq}|{N}|{k}"] = v
    np.savez(out, **save)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return _child(sys.argv[2])
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    t = _cases()
    tmp = tempfile.mkdtemp(prefix="al_chain_spread_")
    try:
        # the cases' states come from the committed build (the test's LP filter uses its labels): the same for every build
        os.environ["VBOC_AL_STATES"] = os.path.join(tmp, "states.npz")
        np.savez(os.environ["VBOC_AL_STATES"], **{f"{nq}|{N}": t.case_states(nq, N, sc)[1] for nq, N, sc in t.CASES})
        runs, skipped = ts.run_variants(tmp, __file__)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    fx = {"variants": [n for n, _ in ts.VARIANTS if n not in skipped], "cases": {}}
    for nq, N, _ in t.CASES:
        get = lambda v, k: runs[v][f"{nq}|{N}|{k}"]
        c = {k: get("committed", k) for k in ("label", "qp_iter", "x", "u")}
        cap = t.al_spec(nq, N).qp_iter_max
        others = [v for v in fx["variants"] if v != "committed"]
        lab = np.zeros(len(c["label"]), bool)
        qit = np.zeros_like(lab)
        at_cap = c["qp_iter"] >= cap
        all1 = c["label"] == 1
        for v in others:
            lab |= get(v, "label") != c["label"]
            qit |= get(v, "qp_iter") != c["qp_iter"]
            at_cap |= get(v, "qp_iter") >= cap
            all1 &= get(v, "label") == 1
        sx = max([float(np.abs(get(v, "x")[all1] - c["x"][all1]).max()) for v in others] + [0.0]) if all1.any() else 0.0
        su = max([float(np.abs(get(v, "u")[all1] - c["u"][all1]).max()) for v in others] + [0.0]) if all1.any() else 0.0
        fx["cases"][f"nq{nq}/N{N}"] = dict(n=int(len(lab)), labels_differ=int(lab.sum()),
                                           labels_differ_not_at_cap=int((lab & ~at_cap).sum()),
                                           qp_iter_differ=int(qit.sum()),
                                           qp_iter_differ_label0=int((qit & (c["label"] == 0)).sum()),
                                           label0=int((c["label"] == 0).sum()), spread_x=sx, spread_u=su)
        print(f"nq{nq}/N{N}", fx["cases"][f"nq{nq}/N{N}"], flush=True)
    with open(out, "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
