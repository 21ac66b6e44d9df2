"""Truncated-solve parity of k_ft (vboc_amd/csrc/ft.h): every IPM and SQP iteration of the free-time and Safe-MPC solver
pinned to the oracle (oracle/vboc_oracle_ft.c), as tests/test_truncated_parity.py does for the boundary-OCP solver.

A solve cut with (nlp_solver_max_iter, qp_solver_iter_max) = (m, q) returns the iterate it stopped at; fsqp() and ft.h
run() stop in the same order, so the cut means the same on both sides, and (0, 1) returns the guess with its cost and row.
Tolerances come from the oracle's own rounding spread alone (tools/trunc_spread_ft.py, tests/golden/trunc_spread_ft.json:
the oracle built with four compiler-flag sets): for a family, a cut and a quantity (max(|dx|, |du|), cost, the row h at
x_N), 100 x the family's largest recorded spread over its groups.  Nothing measured on the GPU enters them.

Families (8 problems per group; the tool's docstring has the laws): ft1 / ft2 / ft3 the free-time pendulum (N in {1, 2, 3,
63, 64, 65, 130}), double and triple (N in {2, 64, 65}; the triple also at N = 3 with every stage-0 component free, with
every terminal state fixed, with infinite velocity path bounds) through vboc_solve_batch_ft - k_ft<1>, k_ft<2>, k_ft<3>;
mpc-rti / mpc-sqp the Safe-MPC hard row and soft-rti / soft-sqp the soft rows at (N, hid) in {(1, 1), (2, 63), (37, 500),
(64, 64), (65, 65), (65, 512)} (and (65, 0) without a row) through vboc_mpc_solve_batch / vboc_mpc_soft_solve_batch -
k_ft<3, true>.  The horizons 63, 64, 65 and 130 are where the kernel's stage loops `k = t; k <= N; k += 64` wrap, the
widths 63, 64, 65, 500, 512 where nn_row's `i = t; i < H; i += 64` does.

Two kinds of problem are not pinned, because the oracle does not agree with itself there; both are found on the CPU by
the tool, never from a GPU result:
  * the free-time pendulum at N <= 3 with q = 100.  Its QP is infeasible (the law keeps q_init 0.05 rad from q_fin, which
    three steps of dt <= 1e-2 cannot cover) and the interior-point iteration count of an infeasible QP depends on the
    compiler flags in every problem (status 4, qp_iter 6 to 75 for the same problem), so no choice of ids gives a group
    within the drop cap.  Those three groups keep the cuts with q <= 5, where the four builds agree.
  * problems whose line search is decided by rounding.  At N <= 2 an SQP with rows often converges in x, u within three
    iterations while its multipliers lag; the next step is ~0, merit(alpha) equals merit(0) to the last digits, and
    `pa < phi0` decides between alpha = 1 (the multipliers jump, status 0) and alpha_min (nothing moves, status 2 at every
    later cut).  The tool therefore also builds the oracle with the acceptance test at phi0 (1 +- 1e-15)
    (VBOC_FT_LS_EPS) and drops a problem whose counters change; the groups at N <= 2 take the first eight ids that
    survive (tools/trunc_spread_ft.py IDS).  With the first eight ids of the pool instead, the GPU gave status 0 after 3
    SQP iterations and 26 / 29 QP iterations on one problem each of soft-sqp/N1/h1/all and soft-sqp/N2/h63/term where the
    committed oracle goes on with status 2 - exactly the counters of the oracle built with the margin +1e-15.

Recorded spreads of the oracle (max over the family's groups; tol is 100 x these):

  cut                  (0,1)    (1,1)    (1,2)    (1,5)    (1,100)  (2,100)  (3,100)  (5,100)  (6,100)
  x, u   ft1           0        3.4e-14  2.0e-12  3.3e-07  1.0e-06  2.8e-06  4.3e-05  3.4e-05  3.4e-06
  x, u   ft2           0        4.8e-14  1.4e-13  1.2e-11  1.6e-11  4.6e-10  5.9e-10  5.7e-09  5.3e-09
  x, u   ft3           0        7.4e-14  2.4e-13  5.0e-10  1.3e-09  8.5e-10  7.7e-10  1.7e-09  1.8e-09
  x, u   mpc-rti       0        1.3e-12  9.9e-13  2.7e-12  8.9e-10
  x, u   mpc-sqp       0        1.3e-12  9.9e-13  2.7e-12  8.9e-10  4.9e-08  9.5e-08  1.4e-07  9.7e-08
  x, u   soft-rti      0        1.7e-12  1.6e-12  6.4e-12  4.4e-10
  x, u   soft-sqp      0        6.4e-13  4.8e-13  1.7e-11  1.3e-10  1.4e-10  2.1e-09  1.5e-09  1.5e-09
  cost   ft1           0        3.6e-15  1.1e-13  4.2e-10  6.1e-11  2.9e-10  1.0e-08  8.9e-09  8.1e-10
  cost   ft2           4.4e-16  1.4e-14  8.7e-14  1.2e-11  1.5e-11  6.8e-11  2.6e-11  1.9e-11  1.9e-11
  cost   ft3           4.4e-16  1.5e-14  2.4e-13  2.0e-11  2.2e-11  2.5e-11  2.0e-11  2.1e-11  2.1e-11
  cost   mpc-rti       1.8e-12  1.1e-11  2.0e-11  1.1e-11  1.7e-10
  cost   mpc-sqp       1.8e-12  1.1e-11  2.0e-11  1.1e-11  1.7e-10  3.6e-08  2.1e-07  9.7e-08  6.3e-09
  cost   soft-rti      3.6e-12  4.0e-09  1.2e-09  9.3e-08  6.4e-10
  cost   soft-sqp      3.6e-12  1.8e-11  1.4e-11  9.3e-08  6.4e-10  2.3e-10  2.3e-10  5.7e-10  5.5e-10
  h      mpc-rti       8.9e-16  2.1e-13  1.5e-13  1.6e-13  6.8e-12
  h      mpc-sqp       8.9e-16  2.1e-13  1.5e-13  1.6e-13  6.8e-12  2.0e-09  1.4e-09  9.8e-10  3.1e-10
  h      soft-rti      1.3e-15  3.4e-13  1.1e-13  1.2e-13  5.8e-12
  h      soft-sqp      1.3e-15  9.4e-14  6.8e-14  2.2e-13  1.9e-12  9.0e-12  6.1e-12  1.1e-11  1.1e-11

Measured on MI355X (max over the family's groups and retained problems against the oracle; every counter equal to the
oracle's and the fixture's; nothing left out):

  cut                  (0,1)    (1,1)    (1,2)    (1,5)    (1,100)  (2,100)  (3,100)  (5,100)  (6,100)
  x, u   ft1           0        2.5e-14  2.0e-12  4.5e-07  7.2e-07  3.9e-06  1.4e-05  1.1e-05  1.1e-06
  cost   ft1           0        1.8e-15  1.1e-13  1.5e-10  9.0e-11  1.8e-10  4.3e-09  3.0e-09  2.8e-10
  x, u   ft2           0        4.3e-14  1.4e-13  1.5e-11  1.6e-11  4.3e-10  4.9e-10  8.0e-09  8.2e-09
  cost   ft2           0        1.4e-14  7.2e-14  1.1e-11  1.6e-11  2.7e-11  1.4e-11  1.1e-11  1.1e-11
  x, u   ft3           0        5.1e-14  1.7e-13  2.0e-10  1.3e-09  4.7e-10  4.3e-10  1.3e-09  1.4e-09
  cost   ft3           0        1.2e-14  1.6e-13  1.6e-11  1.1e-11  2.0e-11  1.9e-11  1.0e-11  1.0e-11
  x, u   mpc-rti       0        6.1e-13  3.3e-13  3.2e-12  1.6e-09
  cost   mpc-rti       1.8e-12  1.6e-11  1.6e-11  9.3e-12  3.0e-10
  h      mpc-rti       0        9.8e-14  8.0e-14  1.1e-13  1.3e-11
  x, u   mpc-sqp       0        6.1e-13  3.3e-13  3.2e-12  1.6e-09  2.4e-08  4.6e-08  6.7e-08  4.7e-08
  cost   mpc-sqp       1.8e-12  1.6e-11  1.6e-11  9.3e-12  3.0e-10  1.7e-08  1.0e-07  4.7e-08  1.0e-09
  h      mpc-sqp       0        9.8e-14  8.0e-14  1.1e-13  1.3e-11  1.0e-09  6.9e-10  4.7e-10  1.7e-10
  x, u   soft-rti      0        1.5e-12  1.6e-12  2.6e-12  2.6e-10
  cost   soft-rti      2.7e-12  5.6e-09  1.8e-09  9.1e-09  1.2e-10
  h      soft-rti      0        2.1e-13  1.7e-13  7.5e-14  4.9e-12
  x, u   soft-sqp/term 0        3.2e-13  2.3e-13  1.7e-11  7.7e-11  8.7e-11  3.1e-09  1.0e-09  9.7e-10
  cost   soft-sqp/term 1.8e-12  1.1e-11  1.5e-11  8.8e-08  1.2e-10  1.2e-10  2.1e-10  3.8e-10  3.1e-10
  h      soft-sqp/term 0        2.8e-14  2.6e-14  2.3e-13  1.4e-12  7.5e-12  5.7e-12  5.2e-12  7.1e-12
  x, u   soft-sqp/all  0        3.3e-13  4.8e-13  1.2e-12  2.1e-11  4.5e-11  4.4e-11  1.5e-10  1.2e-10
  cost   soft-sqp/all  2.7e-12  1.6e-11  1.1e-11  1.1e-11  6.4e-12  1.1e-10  8.6e-12  1.5e-11  2.5e-11
  h      soft-sqp/all  0        4.3e-14  1.9e-14  1.8e-14  2.7e-13  1.1e-12  8.2e-13  2.3e-13  3.2e-13

The row h is the oracle's bit for bit at the guess for every width (hid 1, 63, 64, 65, 500, 512; hard and soft).  The
free-time cost is bit-equal too at the guess: cost() of ft.h sums in the oracle's stage order (a sum across lanes missed
it by 1.2e-14 at N = 63..65 and 2.7e-14 at N = 130, against a recorded spread of 0).  The Safe-MPC cost is summed across
lanes and is within its tolerance, not bit-equal (1.8e-12 against a tolerance of 1.8e-10).  The ragged batch gives ft1's
figures; the tiled batches (2 304 problems on 1 024 workgroups) and the reused handle are bit-equal to their references.
Under the perturbed ipm_tau the smallest deviation at (1, 2) is 5.8e-06 (ft1/N65, tol 2.0e-10), 4.4e-05 (ft3/N65, tol
2.4e-11), 2.2e-06 (mpc-sqp/N65/h65, tol 9.9e-11), 1.4e-06 and 3.5e-06 (soft-sqp/N65/h65 term / all, tol 4.8e-11).
"""
import json
import os
import sys
import time

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import trunc_spread_ft as tf  # noqa: E402

with open(tf.FIXTURE) as _f:
    FX = json.load(_f)
CUTS = tuple(tuple(c) for c in FX["cuts"])
RTI_CUTS = tuple(tuple(c) for c in FX["rti_cuts"])
COUNTERS = tf.COUNTERS
SENTINEL = 7.25e77
TAU = 0.995
SENS_CUT = (1, 2)
SENS_GROUPS = ("ft1/N65", "ft3/N65", "mpc-sqp/N65/h65", "soft-sqp/N65/h65/term", "soft-sqp/N65/h65/all")
# (group, cut) left out of the deviation bars (printed, not asserted; the counters are still asserted): at most two, each
# with a cause named in the module docstring and shown on the CPU by changing the oracle the same way
LEFT_OUT = set()


def _groups(family):
    return [g for g in FX["groups"].values() if g["family"] == family]


def _cuts(g):
    return tuple(tuple(int(v) for v in ck.split(",")) for ck in g["cuts"])


def _keep(g):
    return np.array([i not in g["dropped"] for i in g["ids"]])


class _Reference:
    """The committed oracle on a group at a cut, computed on first use and shared by every test of the module; the
    groups' inputs likewise.  The arrays are read-only."""

    def __init__(self):
        self.inputs, self.runs = {}, {}

    def batch(self, g):
        key = tf.group_key(g)
        if key not in self.inputs:
            b = tf.batch(g)
            for a in b.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self.inputs[key] = b
        return self.inputs[key]

    def run(self, g, cut):
        key = (tf.group_key(g), cut)
        if key not in self.runs:
            r = tf.oracle_solve(oracle, g, self.batch(g), cut)
            for a in r.values():
                a.setflags(write=False)
            self.runs[key] = r
        return self.runs[key]


@pytest.fixture(scope="module")
def reference():
    return _Reference()


# ------------------------------------------------------------------------------------------------ CPU
def test_fixture_covers_the_groups_within_the_drop_cap():
    assert CUTS == tf.CUTS == ((0, 1),) + tf.ts.CUTS and RTI_CUTS == tf.RTI_CUTS
    assert FX["tol_factor"] == tf.TOL_FACTOR == 100.0 and FX["drop_cap"] == tf.DROP_CAP == 1
    assert "committed" in FX["variants"] and len(FX["variants"]) >= 3
    assert [tf.group_key(g) for g in tf.groups()] == list(FX["groups"])
    assert {g["family"] for g in FX["groups"].values()} == set(tf.FAMILIES)
    for g, e in zip(tf.groups(), FX["groups"].values()):
        key = tf.group_key(g)
        assert all(e[k] == g[k] for k in g), (g, e)
        assert len(e["ids"]) == tf.PER == 8 and len(e["dropped"]) <= tf.DROP_CAP and set(e["dropped"]) <= set(e["ids"])
        assert _cuts(e) == tf.cuts_of(g), key
        keep = _keep(e)
        for cut in _cuts(e):
            c = e["cuts"][tf.cut_key(cut)]
            assert all(len(c[k]) == tf.PER for k in COUNTERS)
            assert ("spread_h" in c) == (g["kind"] != "ft")
            for what in ("spread", "spread_cost") + (("spread_h",) if g["kind"] != "ft" else ()):
                assert np.isfinite(c[what]) and 0.0 <= c[what] < 1e-3, (key, cut, what, c[what])
            # the guess comes back untouched at (0, 1), and wherever no retained problem took a step (a first QP that
            # fails); every other iterate differs between the builds
            stepped = np.array(c["sqp_iter"])[keep & (np.array(c["status"]) != 5)]
            if cut == (0, 1) or not stepped.any():
                assert c["spread"] == 0.0, (key, cut)
            else:
                assert c["spread"] > 0.0, (key, cut)
    # the only groups with a shortened cut list: the infeasible short pendulum horizons (module docstring)
    short = [tf.group_key(g) for g in tf.groups() if tf.cuts_of(g) not in (CUTS, RTI_CUTS)]
    assert short == ["ft1/N1", "ft1/N2", "ft1/N3"]
    for fam in tf.FAMILIES:
        for cut in (RTI_CUTS if fam.endswith("rti") else CUTS)[1:]:
            assert tf.tol(FX, fam, cut) > 0.0


def test_every_family_wraps_the_wave_and_has_a_short_horizon():
    for fam in tf.FAMILIES:
        Ns = [g["N"] for g in _groups(fam)]
        assert max(Ns) >= 65 and min(Ns) <= 2, (fam, Ns)
    assert {g["N"] for g in _groups("ft1")} >= {1, 63, 64, 65, 130}
    for fam in tf.FAMILIES[3:]:
        assert {g["hid"] for g in _groups(fam)} >= {1, 63, 64, 65, 500, 512}


def test_oracle_reproduces_the_fixture_counters(reference):
    """A drift of the committed oracle, or of an input generator, shows here and not on the GPU machine."""
    bad = []
    for g in FX["groups"].values():
        keep = _keep(g)
        for cut in _cuts(g):
            r, e = reference.run(g, cut), g["cuts"][tf.cut_key(cut)]
            for k in COUNTERS:
                if not np.array_equal(r[k][keep], np.array(e[k])[keep]):
                    bad.append((tf.group_key(g), cut, k, r[k].tolist(), e[k]))
    assert not bad, bad


def test_oracle_moves_with_ipm_tau(reference):
    """The premise of the GPU can-fail test, on the oracle alone: under ipm_tau = 0.995 (1 + 1e-6) every retained problem
    of the sensitivity groups moves at the cut (1, 2) by more than 1e4 x its family's tolerance there."""
    low = {}
    for key in SENS_GROUPS:
        g = FX["groups"][key]
        moved = tf.oracle_solve(oracle, g, reference.batch(g), SENS_CUT, ipm_tau=TAU * (1.0 + 1e-6))
        dev = tf.deviation(g, moved, reference.run(g, SENS_CUT))[_keep(g)]
        low[key] = (float(dev.min()), 1e4 * tf.tol(FX, g["family"], SENS_CUT))
    print("\n" + "\n".join(f"{k}: smallest move {a:.1e}, 1e4 tol {b:.1e}" for k, (a, b) in low.items()))
    assert all(a > b for a, b in low.values()), low


# ------------------------------------------------------------------------------------------------ GPU
MPC_OPTS = dict(levenberg_marquardt=1e-2, nlp_solver_tol_stat=1e-6, qp_solver_tol_stat=1e-8)   # test_safempc.py _gpu


def _ft_solver(nq, **options):
    from vboc_amd import lib
    return lib.Solver(nq, tf.FT_NMAX, slots=256, **options)


def _mpc_solver(N, **options):
    from vboc_amd import lib
    return lib.Solver(3, N, slots=256, **dict(MPC_OPTS, **options))


def _set_cut(s, cut):
    s.set_option("nlp_solver_max_iter", cut[0])
    s.set_option("qp_solver_iter_max", cut[1])


def _pad(b, nmax, fill):
    """A free-time batch with its guesses padded to nmax; the rows beyond the batch's own horizon hold `fill`."""
    out = dict(b)
    for k in ("x_guess", "u_guess"):
        a = b[k]
        pad = np.full((a.shape[0], nmax + (k == "x_guess") - a.shape[1], a.shape[2]), fill)
        out[k] = np.concatenate([a, pad], axis=1)
    return out


def _solve_ft(s, b, cut):
    _set_cut(s, cut)
    return s.solve_host(b, free_time=True)


def _solve_mpc(s, g, b, cut, rows=None):
    """The group's Safe-MPC call (hard row, or the soft rows of g['weights']) on the problems `rows` of its inputs."""
    import torch
    _set_cut(s, cut)
    rows = np.arange(len(g["ids"])) if rows is None else np.asarray(rows)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")
    prm = [T(p) for p in b["params"]] if b["params"] is not None else None
    soft = None
    if g["kind"] == "soft":
        per = g["weights"] == "all"
        soft = dict(margin=tf.MARGIN, Zl=T(np.tile(tf.soft_Zl(g["N"], g["weights"]), (rows.size, 1))),
                    W=T(b["W"][rows]) if per else None, We=T(b["We"][rows]) if per else None)
    out = s.mpc_solve_device(b["spec"], T(b["x0"][rows]), T(b["xg"][rows]), T(b["ug"][rows]), prm, tf.MEAN, tf.STD,
                             rti=g["rti"], soft=soft)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


def _check(g, gpu, ref, cut, fails, rows=None, tag=""):
    """The assertions on one group at one cut (rows: the group's problems inside a larger batch); returns the largest
    deviations (x / u, cost, h).  Failures are collected, so one run reports every (group, cut) that misses."""
    key = tf.group_key(g)
    what = f"{key}{tag} {cut}"
    out = (key, cut) in LEFT_OUT
    rows = slice(None) if rows is None else rows
    keep, N, fam = _keep(g), g["N"], g["family"]
    e = g["cuts"][tf.cut_key(cut)]
    res = {k: gpu[k][rows] for k in COUNTERS + ("cost",) + (("h",) if "h" in ref else ())}
    res["x"], res["u"] = gpu["x"][rows][:, :N + 1], gpu["u"][rows][:, :N]
    for k in COUNTERS:
        if not (np.array_equal(res[k][keep], ref[k][keep]) and np.array_equal(res[k][keep], np.array(e[k])[keep])):
            fails.append(f"{what} {k}: gpu {res[k].tolist()} oracle {ref[k].tolist()} fixture {e[k]}")
    nan_g, nan_r = np.isnan(res["cost"])[keep], np.isnan(ref["cost"])[keep]
    if not np.array_equal(nan_g, nan_r):
        fails.append(f"{what}: NaN costs differ: gpu {res['cost']} oracle {ref['cost']}")
    m = keep & tf.solved(ref)          # a rejected structure (status 5) returns no iterate
    worst = dict(spread=0.0, spread_cost=0.0, spread_h=0.0)
    if not m.any():
        return worst
    devs = dict(spread=tf.deviation(g, res, ref)[m], spread_cost=np.abs(res["cost"] - ref["cost"])[m])
    if "h" in ref:
        devs["spread_h"] = np.abs(res["h"] - ref["h"])[m]
    for k, d in devs.items():
        tol = tf.tol(FX, fam, cut, k)
        d = d[~np.isnan(d)] if k == "spread_cost" else d
        if out:
            print(f"\nleft out: {what} {k} {d.max():.1e} (tol {tol:.1e})")
        elif d.size and not d.max() <= tol:
            fails.append(f"{what} {k}: {d.max():.3e} > tol {tol:.3e} (per problem {d})")
        elif d.size:
            worst[k] = float(d.max())
    return worst


def _report(name, cuts, worst):
    for k, label in (("spread", "x, u"), ("spread_cost", "cost"), ("spread_h", "h")):
        if k == "spread_h" and name.startswith("ft"):
            continue
        print(f"  {label:6s} {name:13s} " + "  ".join(f"{worst[c][k]:.1e}" if worst[c][k] else "0      " for c in cuts))


def _family_parity(family, reference, weights=None):
    cuts = RTI_CUTS if family.endswith("rti") else CUTS
    fails = []
    worst = {c: dict(spread=0.0, spread_cost=0.0, spread_h=0.0) for c in cuts}
    s = _ft_solver(_groups(family)[0]["nq"]) if family.startswith("ft") else None
    try:
        for g in _groups(family):
            if weights is not None and g["weights"] != weights:
                continue
            b = reference.batch(g)
            if s is None:
                sm = _mpc_solver(g["N"])
            else:
                bp = _pad(b, tf.FT_NMAX, SENTINEL)
            try:
                for cut in _cuts(g):
                    if s is None:
                        gpu = _solve_mpc(sm, g, b, cut)
                    else:
                        gpu = _solve_ft(s, bp, cut)
                        N = g["N"]      # the rows beyond the horizon: the input's, bit for bit
                        if not (np.array_equal(gpu["x"][:, N + 1:], bp["x_guess"][:, N + 1:])
                                and np.array_equal(gpu["u"][:, N:], bp["u_guess"][:, N:])):
                            fails.append(f"{tf.group_key(g)} {cut}: rows beyond N differ from the input")
                    w = _check(g, gpu, reference.run(g, cut), cut, fails)
                    worst[cut] = {k: max(v, w[k]) for k, v in worst[cut].items()}
            finally:
                if s is None:
                    sm.close()
    finally:
        if s is not None:
            s.close()
    print()
    _report(family + ("" if weights is None else "/" + weights), cuts, worst)
    assert not fails, "\n".join(fails)


# the soft-row SQP family runs as one case per weighting: together they take longer than a test here may
CASES = [(f, None) for f in tf.FAMILIES[:-1]] + [("soft-sqp", w) for w in tf.SOFT_WEIGHTS]


@pytest.mark.gpu
@pytest.mark.parametrize("family,weights", CASES, ids=[f if w is None else f"{f}-{w}" for f, w in CASES])
def test_truncated_solves_follow_the_oracle(family, weights, reference):
    t0 = time.perf_counter()
    _family_parity(family, reference, weights)
    print(f"  {family} {weights or ''}: {time.perf_counter() - t0:.1f} s")


@pytest.mark.gpu
def test_row_at_the_guess_is_the_oracles_bit_for_bit(reference):
    """At the cut (0, 1) both sides evaluate the row and the cost at the same x, the guess.  nn_row (ft.h) restates the
    oracle's row operation for operation with contraction off, so h must be the oracle's to the last bit at every width
    on either side of a 64-lane wrap, hard and soft.  The cost is summed across lanes (ft_wsum) where the oracle sums
    in stage order: it is within its tolerance, not bit-equal (printed per group)."""
    fails, seen = [], set()
    for fam in ("mpc-sqp", "soft-sqp"):
        for g in _groups(fam):
            if g["hid"] == 0:
                continue
            seen.add(g["hid"])
            s = _mpc_solver(g["N"])
            try:
                gpu = _solve_mpc(s, g, reference.batch(g), (0, 1))
            finally:
                s.close()
            ref = reference.run(g, (0, 1))
            dh = np.abs(gpu["h"] - ref["h"]).max()
            dc = np.abs(gpu["cost"] - ref["cost"]).max()
            print(f"\n{tf.group_key(g)}: max |dh| {dh:.1e}, max |dcost| {dc:.1e}"
                  f" ({'bit-equal' if np.array_equal(gpu['cost'], ref['cost']) else 'within tol'})")
            if not np.array_equal(gpu["h"], ref["h"]):
                fails.append(f"{tf.group_key(g)}: h differs from the oracle's by {dh:.3e}")
            if not (np.array_equal(gpu["x"], ref["x"]) and np.array_equal(gpu["u"], ref["u"])):
                fails.append(f"{tf.group_key(g)}: the guess did not come back")
            if not dc <= tf.tol(FX, fam, (0, 1), "spread_cost"):
                fails.append(f"{tf.group_key(g)}: |dcost| {dc:.3e} > tol {tf.tol(FX, fam, (0, 1), 'spread_cost'):.3e}")
    assert seen == {1, 63, 64, 65, 500, 512}
    assert not fails, "\n".join(fails)


def _ragged(reference, fill):
    """The pendulum's seven horizons as one free-time batch, nmax = 130; guess rows beyond N[b] hold `fill`."""
    gs = _groups("ft1")
    parts = [_pad(reference.batch(g), tf.FT_NMAX, fill) for g in gs]
    return gs, {k: np.concatenate([p[k] for p in parts]) for k in tf.ts.KEYS}


def _same(a, b, N, idx=None, what=""):
    """Counters, cost and x, u up to N[b] of result a bit-equal to result b (rows idx of b)."""
    idx = np.arange(len(N)) if idx is None else idx
    for k in COUNTERS + ("cost",):
        np.testing.assert_array_equal(a[k], b[k][idx], err_msg=f"{what} {k}")
    for n in np.unique(N):
        r = np.flatnonzero(N == n)
        np.testing.assert_array_equal(a["x"][r, :n + 1], b["x"][idx[r], :n + 1], err_msg=f"{what} x, N = {n}")
        np.testing.assert_array_equal(a["u"][r, :n], b["u"][idx[r], :n], err_msg=f"{what} u, N = {n}")


@pytest.mark.gpu
def test_ragged_batch_ignores_and_keeps_the_rows_beyond_the_horizon(reference):
    gs, bs = _ragged(reference, SENTINEL)
    _, bz = _ragged(reference, 0.0)
    assert bs["x_guess"].shape == (56, 131, 3) and sorted(set(bs["N"].tolist())) == [1, 2, 3, 63, 64, 65, 130]
    s = _ft_solver(1)
    fails = []
    try:
        for cut in CUTS:
            gsent, gzero = _solve_ft(s, bs, cut), _solve_ft(s, bz, cut)
            _same(gsent, gzero, bs["N"], what=f"{cut} sentinel against zero padding")
            for j, g in enumerate(gs):
                rows, N = slice(tf.PER * j, tf.PER * j + tf.PER), g["N"]
                for gpu, b in ((gsent, bs), (gzero, bz)):
                    np.testing.assert_array_equal(gpu["x"][rows, N + 1:], b["x_guess"][rows, N + 1:], err_msg=f"{cut} N={N}")
                    np.testing.assert_array_equal(gpu["u"][rows, N:], b["u_guess"][rows, N:], err_msg=f"{cut} N={N}")
                if cut in _cuts(g):
                    _check(g, gsent, reference.run(g, cut), cut, fails, rows=rows, tag=" ragged")
    finally:
        s.close()
    assert not fails, "\n".join(fails)


TILED = 2304          # 2.25 x the kernel's grid of 1024 workgroups: every region serves two or three problems
REUSE_CUTS = ((1, 5), (2, 100))


def _tiled_pendulum(reference):
    """The ragged batch's 56 problems tiled to TILED, each tile ordered from the longest horizon to the shortest, so a
    region's next problem is usually shorter than what its records held before."""
    _, b = _ragged(reference, SENTINEL)
    order = np.argsort(-b["N"], kind="stable")
    idx = order[np.arange(TILED) % order.size]
    return b, idx, {k: np.ascontiguousarray(b[k][idx]) for k in tf.ts.KEYS}


@pytest.mark.gpu
def test_a_result_does_not_depend_on_what_its_region_held_before(reference):
    """(a) 2 304 free-time problems on 1 024 workgroups: every copy bit-equal to the 56-problem run.  (c) the same with 16
    problems of the first wave of the grid replaced by ones whose control guess is 1e160: those end with a status != 0 and
    every other problem is bit-equal to (a), so neither a region's records nor FtShared carry anything over."""
    b56, idx, bt = _tiled_pendulum(reference)
    poisoned = 3 + 61 * np.arange(16)
    bp = {k: a.copy() for k, a in bt.items()}
    bp["u_guess"][poisoned] = 1e160
    clean = np.setdiff1d(np.arange(TILED), poisoned)
    s = _ft_solver(1)
    try:
        for cut in REUSE_CUTS:
            base, tiled, pois = _solve_ft(s, b56, cut), _solve_ft(s, bt, cut), _solve_ft(s, bp, cut)
            _same(tiled, base, bt["N"], idx, what=f"{cut} tiled against the 56-problem run")
            assert (pois["status"][poisoned] != 0).all(), pois["status"][poisoned]
            sub = lambda r: {k: r[k][clean] for k in r}
            _same(sub(pois), tiled, bt["N"][clean], clean, what=f"{cut} beside poisoned problems")
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 63), (65, 65)])
def test_soft_rows_do_not_depend_on_what_their_region_held_before(shape, reference):
    """(b) the soft rows (SQP_RTI, cut (1, 100), both weightings) tiled to 2 304 problems: every copy bit-equal to the
    8-problem run - the row fields of the records, the slacks and the network buffers of FtShared included."""
    cut = (1, 100)
    for g in _groups("soft-rti"):
        if (g["N"], g["hid"]) != shape:
            continue
        b = reference.batch(g)
        s = _mpc_solver(g["N"])
        try:
            base = _solve_mpc(s, g, b, cut)
            idx = np.arange(TILED) % tf.PER
            tiled = _solve_mpc(s, g, b, cut, rows=idx)
        finally:
            s.close()
        for k in COUNTERS + ("cost", "h", "x", "u"):
            np.testing.assert_array_equal(tiled[k], base[k][idx], err_msg=f"{tf.group_key(g)} {k}")
        fails = []
        _check(g, base, reference.run(g, cut), cut, fails)
        assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_a_handle_gives_a_fresh_handles_result_after_other_record_sizes(reference):
    """One handle runs the free-time triple at N = 65, the soft Safe-MPC rows at (65, 65) (a longer stage record: the
    regions are reallocated) and the free-time triple at N = 2 (the short record again, in the larger allocation): each
    result bit-equal to a fresh handle's."""
    from vboc_amd import lib
    g65, g2 = FX["groups"]["ft3/N65"], FX["groups"]["ft3/N2"]
    gm = FX["groups"]["soft-rti/N65/h65/all"]
    ft_cut, mpc_cut = (2, 100), (1, 100)

    def fresh_ft(g):
        s = _ft_solver(3)
        try:
            return _solve_ft(s, reference.batch(g), ft_cut)
        finally:
            s.close()

    s = _mpc_solver(gm["N"])
    try:
        want_m = _solve_mpc(s, gm, reference.batch(gm), mpc_cut)
    finally:
        s.close()
    want65, want2 = fresh_ft(g65), fresh_ft(g2)
    s = lib.Solver(3, tf.FT_NMAX, slots=256)
    try:
        defaults = {k: s.get_option(k) for k in MPC_OPTS}
        got65 = _solve_ft(s, reference.batch(g65), ft_cut)
        for k, v in MPC_OPTS.items():
            s.set_option(k, v)
        got_m = _solve_mpc(s, gm, reference.batch(gm), mpc_cut)
        for k, v in defaults.items():
            s.set_option(k, v)
        got2 = _solve_ft(s, reference.batch(g2), ft_cut)
    finally:
        s.close()
    for name, got, want in (("ft3/N65", got65, want65), ("soft (65, 65)", got_m, want_m), ("ft3/N2", got2, want2)):
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name} {k}")
    fails = []
    _check(g65, got65, reference.run(g65, ft_cut), ft_cut, fails)
    _check(gm, got_m, reference.run(gm, mpc_cut), mpc_cut, fails)
    _check(g2, got2, reference.run(g2, ft_cut), ft_cut, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_a_relative_change_of_1e_6_in_ipm_tau_misses_the_tolerance(reference):
    """The GPU at ipm_tau = 0.995 (1 + 1e-6) against the oracle at 0.995: every retained problem of the sensitivity
    groups misses tol at the cut (1, 2), so the parity test can fail."""
    for key in SENS_GROUPS:
        g = FX["groups"][key]
        b = reference.batch(g)
        tol = tf.tol(FX, g["family"], SENS_CUT)
        opt = dict(ipm_tau=TAU * (1.0 + 1e-6))
        s = _ft_solver(g["nq"], **opt) if g["kind"] == "ft" else _mpc_solver(g["N"], **opt)
        try:
            gpu = _solve_ft(s, b, SENS_CUT) if g["kind"] == "ft" else _solve_mpc(s, g, b, SENS_CUT)
        finally:
            s.close()
        dev = tf.deviation(g, gpu, reference.run(g, SENS_CUT))[_keep(g)]
        print(f"\n{key}: perturbed tau: smallest deviation {dev.min():.1e}, tol {tol:.1e}")
        assert np.all(dev > tol), (key, dev, tol)
