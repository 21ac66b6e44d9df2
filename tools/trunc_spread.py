"""The oracle's own rounding spread on truncated solves: the source of every tolerance of
tests/test_truncated_parity.py.  CPU only.

A solve cut with (nlp_solver_max_iter, qp_solver_iter_max) = (m, q) returns the iterate it stopped at (status 2;
oracle/vboc_oracle.c sqp(), coop.h run()), a QP stopped at its cap is not fatal and its step is taken.  So the cut
(1, 1) is one IPM iteration, one line search and one step, and nothing later can repair an error in it.  How far may
two correct FP64 implementations differ there?  This tool answers with the oracle alone: it copies oracle/ to a
temporary directory, builds it with several compiler-flag sets that re-associate or contract its arithmetic (VARIANTS;
a set that does not build is skipped and listed), runs every variant in a child process (VBOC_ORACLE_LIB) on every
group and cut below, and writes to tests/golden/trunc_spread.json, per group and cut:

  * the ids, and per problem the committed build's status, sqp_iter and qp_iter;
  * spread: the max over variants and retained problems of max(|dx|, |du|) against the committed build over rows
    0..N (absolute; the values are of order 10).  No trajectory is stored.

A problem whose status, sqp_iter or qp_iter differ between variants at any cut is dropped from its group and listed
(dropped); at most DROP_CAP of a group's problems may go, else the tool fails: choose other ids, do not raise the cap.

The tolerance rule (tol()): for a system and a cut, TOL_FACTOR x the largest recorded spread of that system at that
cut over its horizons.  The factor covers that a handful of flag sets over 8 problems per horizon under-sample the
maximum, and that the GPU differs from the oracle by more re-associations than a contraction switch does (MFMA
accumulation order, closed-form Ru^-1, cross-lane reduction trees, device sin / cos).  Nothing measured on the GPU
enters it.

usage: python tools/trunc_spread.py [--out FILE]      (regenerates the fixture; the discrete counters must not change)
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "trunc_spread.json")

CUTS = ((1, 1), (1, 2), (1, 5), (1, 100), (2, 100), (3, 100), (5, 100), (6, 100))
PER = 8                 # problems per group
DROP_CAP = 1            # of them, how many may be dropped
TOL_FACTOR = 100.0

# (system, nq, initial-condition law of vboc_amd.ics, horizons); the UR5 and the Cartesian double pendulum run at
# their laws' own horizon
SYSTEMS = (("triple", 3, "data_generation_ics", (1, 2, 3, 4, 7, 9, 100)),
           ("double", 2, "data_generation_ics", (1, 2, 3, 7, 100)),
           ("pendulum", 1, "heldout_ics", (1, 2, 3, 7, 100)),
           ("ur5", 4, "ur5_ics", (100,)),
           ("cartesian", 2, "cartesian_ics", (100,)))

BASE = "-O2 -std=c99 -fPIC -Wall -Wextra -fopenmp -ffp-contract=off"     # oracle/Makefile
VARIANTS = (("committed", BASE),
            ("contract", "-O2 -std=c99 -fPIC -fopenmp -ffp-contract=fast -march=native"),
            ("assoc", "-O3 -std=c99 -fPIC -fopenmp -ffp-contract=off -fassociative-math -fno-signed-zeros "
                      "-fno-trapping-math"),
            ("x87", "-O2 -std=c99 -fPIC -fopenmp -ffp-contract=off -mfpmath=387"))

KEYS = ("N", "x_guess", "u_guess", "p", "lbx", "ubx", "lbu", "ubu", "lbx0", "ubx0", "lbxe", "ubxe")


# Groups whose ids are not their system's consecutive block.  The triple at N = 1: of the ids 0..12, the first eight
# whose first interior-point step is cut by the fraction-to-the-boundary rule, alpha = min(1, ipm_tau amax) < 1 in the
# committed oracle.  The others (0, 1, 3, 4, 10) take the full step, so ipm_tau does not enter their (1, 1) iterate
# and the sensitivity test of tests/test_truncated_parity.py, which asks every triple problem to move under a change
# of ipm_tau, could not hold for them (test_oracle_moves_with_ipm_tau there checks the choice on the CPU).
IDS = {("triple", 1): (2, 5, 6, 7, 8, 9, 11, 12)}


def groups():
    """Every (system, horizon) group: dict(system, nq, ics, N, ids).  A system's horizons take consecutive id blocks."""
    out = []
    for name, nq, law, horizons in SYSTEMS:
        for j, N in enumerate(horizons):
            ids = IDS.get((name, N), range(PER * j, PER * j + PER))
            out.append(dict(system=name, nq=nq, ics=law, N=N, ids=list(ids)))
    return out


def group_key(g):
    return f"{g['system']}/N{g['N']}"


def cut_key(cut):
    return f"{cut[0]},{cut[1]}"


def batch(g):
    """The group's input arrays (vboc_amd.ics layout)."""
    from vboc_amd import ics
    ids = np.asarray(g["ids"])
    if g["ics"] in ("ur5_ics", "cartesian_ics"):
        b = getattr(ics, g["ics"])(ids, N=g["N"])
    else:
        b = getattr(ics, g["ics"])(g["nq"], ids, N=g["N"])
    return {k: b[k] for k in KEYS}


def oracle_opts(oracle, g, cut, **kw):
    """The oracle's options of the group (the UR5's levenberg_marquardt, the Cartesian circle) at a cut."""
    o = dict(max_iter=cut[0], qp_max_iter=cut[1])
    if g["nq"] == 4:
        o["lm"] = 1e-2
    if g["system"] == "cartesian":
        o.update(oracle.cartesian_opts())
    o.update(kw)
    return oracle.default_opts(**o)


def oracle_solve(oracle, g, b, cut, **kw):
    """dict(status, sqp_iter, qp_iter, cost, x, u) of the loaded oracle library on the group at the cut."""
    x, u, r = oracle.solve_batch(g["nq"], *[b[k] for k in KEYS], opts=oracle_opts(oracle, g, cut, **kw),
                                 nthreads=len(g["ids"]))
    return dict(status=np.array(r["status"]), sqp_iter=np.array(r["sqp_iter"]), qp_iter=np.array(r["qp_iter"]),
                cost=np.array(r["cost"]), x=x, u=u)


def deviation(g, a, c):
    """Per problem max(|dx|, |du|) over rows 0..N between two result sets of the group (full [B, N+1, .] arrays)."""
    N = g["N"]
    dx = np.abs(a["x"][:, :N + 1] - c["x"][:, :N + 1]).reshape(len(g["ids"]), -1).max(axis=1)
    du = np.abs(a["u"][:, :N] - c["u"][:, :N]).reshape(len(g["ids"]), -1).max(axis=1)
    return np.maximum(dx, du)


def tol(fixture, system, cut):
    """TOL_FACTOR x the largest recorded spread of the system at the cut over its horizons."""
    s = [e["cuts"][cut_key(cut)]["spread"] for e in fixture["groups"].values() if e["system"] == system]
    return TOL_FACTOR * max(s)


def _child(out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    import oracle
    assert os.environ.get("VBOC_ORACLE_LIB") and oracle.LIB == os.environ["VBOC_ORACLE_LIB"]
    save = {}
    for g in groups():
        b = batch(g)
        for cut in CUTS:
            r = oracle_solve(oracle, g, b, cut)
            for k, v in r.items():
                save[f"{group_key(g)}|{cut_key(cut)}|{k}"] = v
    np.savez(out, **save)


def run_variants(tmp, script, variants=None):
    """Copy oracle/ into tmp once per flag set of `variants` (default VARIANTS), build it, and run `script --child OUT.npz` on each build
    (VBOC_ORACLE_LIB).  Returns ({variant: the npz}, [the variants that do not build])."""
    runs, skipped = {}, []
    for name, flags in variants or VARIANTS:
        d = os.path.join(tmp, name)
        shutil.copytree(os.path.join(ROOT, "oracle"), os.path.join(d, "oracle"),
                        ignore=shutil.ignore_patterns("*.so", "__pycache__", "_ref"))
        os.makedirs(os.path.join(d, "vboc_amd", "csrc"))     # vboc_oracle.c includes the arm's parameters from there
        shutil.copy(os.path.join(ROOT, "vboc_amd", "csrc", "ur5_params.h"), os.path.join(d, "vboc_amd", "csrc"))
        mk = subprocess.run(["make", "-s", "-C", os.path.join(d, "oracle"), f"CFLAGS={flags}"],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if mk.returncode != 0:
            if name == "committed":
                raise RuntimeError(mk.stdout)
            skipped.append(name)
            print(f"variant {name} does not build, skipped:\n{mk.stdout[-400:]}", file=sys.stderr)
            continue
        npz = os.path.join(d, "out.npz")
        env = dict(os.environ, VBOC_ORACLE_LIB=os.path.join(d, "oracle", "libvboc_oracle.so"))
        subprocess.check_call([sys.executable, os.path.abspath(script), "--child", npz], env=env)
        runs[name] = np.load(npz)
    return runs, skipped


def write_fixture(out, fx):
    """The fixture as JSON, one line per group and cut."""
    with open(out, "w") as f:
        head = {k: v for k, v in fx.items() if k != "groups"}
        f.write("{\n" + "".join(f" {json.dumps(k)}: {json.dumps(v)},\n" for k, v in head.items()))
        f.write(' "groups": {\n')
        for i, (gk, e) in enumerate(fx["groups"].items()):
            f.write(f"  {json.dumps(gk)}: {{\n")
            f.write("".join(f"   {json.dumps(k)}: {json.dumps(v)},\n" for k, v in e.items() if k != "cuts"))
            cuts = ",\n".join(f"    {json.dumps(ck)}: {json.dumps(cv)}" for ck, cv in e["cuts"].items())
            f.write('   "cuts": {\n' + cuts + "\n   }\n  }" + ("," if i + 1 < len(fx["groups"]) else "") + "\n")
        f.write(" }\n}\n")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return _child(sys.argv[2])
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    tmp = tempfile.mkdtemp(prefix="trunc_spread_")
    try:
        runs, skipped = run_variants(tmp, __file__)
        base = runs["committed"]
        fx = dict(cuts=[list(c) for c in CUTS], tol_factor=TOL_FACTOR, drop_cap=DROP_CAP,
                  variants={n: f for n, f in VARIANTS if n in runs}, skipped_variants=skipped, groups={})
        for g in groups():
            B = len(g["ids"])
            get = lambda run, cut, k: run[f"{group_key(g)}|{cut_key(cut)}|{k}"]
            keep = np.ones(B, bool)
            for cut in CUTS:
                for run in runs.values():
                    for k in ("status", "sqp_iter", "qp_iter"):
                        keep &= get(run, cut, k) == get(base, cut, k)
            dropped = [g["ids"][i] for i in np.where(~keep)[0]]
            if len(dropped) > DROP_CAP:
                raise RuntimeError(f"{group_key(g)}: {len(dropped)} problems with counters that depend on the build "
                                   f"({dropped}); choose other ids")
            e = dict(g, dropped=dropped, cuts={})
            for cut in CUTS:
                a = {k: get(base, cut, k) for k in ("x", "u")}
                spread = 0.0
                for run in runs.values():
                    d = deviation(g, a, {k: get(run, cut, k) for k in ("x", "u")})
                    spread = max(spread, float(d[keep].max()))
                e["cuts"][cut_key(cut)] = dict(status=get(base, cut, "status").tolist(),
                                               sqp_iter=get(base, cut, "sqp_iter").tolist(),
                                               qp_iter=get(base, cut, "qp_iter").tolist(), spread=spread)
            fx["groups"][group_key(g)] = e
        write_fixture(out, fx)
        for name in dict.fromkeys(s[0] for s in SYSTEMS):
            print(name, " ".join(f"{cut_key(c)}: {tol(fx, name, c) / TOL_FACTOR:.1e}" for c in CUTS))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
