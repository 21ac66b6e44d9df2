"""The sweeps' per-stage vectors in LDS rows (coop.h, VBOC_FUSE bits 32 and 64): in the triple's MFMA data-generation
kernels the forward sweeps' and the corrector vector sweep's constant C travels through the staging rows XS, and k_f /
k_f - M nu through three more words of each row, instead of the stage record.  Same operations in the same order, so
results are those of the parent commit bit for bit.  GPU tests:

  * one ragged wave-solver batch (4 problems per horizon, ids 4j .. 4j+3) at the horizons where the grouped sweeps
    can go wrong: N = 2 (one interior stage: a partial group), 3, 4 (exactly one 3-stage group), 5 (a group plus a
    partial one), 7 (two groups), 8, 63 (the stage-parallel trips exactly full), 64 (they spill one lane), 100, 112
    (the workload's horizons), 119, 120 (the last rows and the top group's over-read) - bit for bit against the
    fixture tests/golden/lds_vectors_parent.npz recorded from the parent commit's library (tools/
    record_lds_vectors.py; the fixture ships the inputs), against the same library with factor_mfma = 0 at
    test_factor_solve.py's bars, and against itself;
  * the device data-generation and testing loops (k_dg<3, true>, k_ts<3, true>: the kernels that run the new passes),
    bit for bit against the parent's rows in the same fixture: at the workload's start horizon 100, and started at
    2, 3, 5 (solves at N = 2 .. 14: the partial, one-group and two-group sweeps), 51, 63 (N = 51 .. 75: the
    stage-parallel trips full at 63 and spilling one lane from 64) and 108 (N = 108 .. 120: the last rows and the
    top group's over-read) - a problem solves at its start horizon .. + 9 and verifies at up to + 12;
  * the same two loops at start 108 on ONE workgroup (wave_groups = 1, no speculative or parked jobs): each problem's
    first solves at N = 108 follow the previous problem's longest ones, failed solves among them, on the same LDS
    rows and slack - bit for bit against the parent;
  * poisoned problems (a control guess of 1e160) with N = 120 followed on the same workgroup by N = 100 problems in
    the wave solver: stale non-finite words must not reach them.

Reach: k_wave<3, true>, the kernel behind solve_host, keeps the parent's passes (its code size is pinned by
tests/test_isa_guard.py and the new passes do not fit its alignment step), so the ragged batch and the poisoned
problems pin that kernel to the parent.  The LDS-row passes are reached through the device loops, which take their
inputs from the problem id alone: a poisoned guess cannot be handed to them, so stale rows are covered there by the
one-workgroup run (the loops' own failing solves - horizon extensions that stop at the iteration cap or on a QP
failure - precede shorter ones) and by tests/test_dg_device.py / test_drivers.py.

Measured on MI355X (profiles/r08_pytest_lds_vectors.log): against factor_mfma = 0 status agreement 48 / 48,
SQP-iteration agreement 48 / 48, 46 converged on both (one problem each at N = 8 and N = 63 stops at the 200-iteration
cap on both), |dcost| median 2.3e-13, max 1.9e-11, |dx0| median 1.4e-13, max 1.6e-11; the poisoned problems end with
status 4, the eight others converge and equal the clean run; 368 data-generation rows and 12 testing rows equal the
parent's.  The whole file takes 5 s.
"""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HORIZONS = (2, 3, 4, 5, 7, 8, 63, 64, 100, 112, 119, 120)
PER = 4
NMAX = 120
MAX_ITER = 200
IN_KEYS = ("N", "x_guess", "u_guess", "p", "lbx", "ubx", "lbu", "ubu", "lbx0", "ubx0", "lbxe", "ubxe")
OUT_KEYS = ("status", "sqp_iter", "qp_iter", "cost", "x", "u")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lds_vectors_parent.npz")


def _sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def _gpu(b, slots=1024, **opts):
    from vboc_amd import lib
    s = lib.Solver(3, NMAX, slots=slots)
    for k, v in opts.items():
        s.set_option(k, v)
    try:
        g = s.solve_host(b)
        g["last_groups"] = s.get_option("last_groups")
        return g
    finally:
        s.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(golden):
    b = {k: np.ascontiguousarray(golden["in_" + k]) for k in IN_KEYS}
    assert b["N"].tolist() == [N for N in HORIZONS for _ in range(PER)]
    opts = dict(nlp_solver_max_iter=MAX_ITER, coop_threshold=8192, wave_all=1)
    return {"b": b, "mfma": _gpu(b, factor_mfma=1, **opts), "again": _gpu(b, factor_mfma=1, **opts),
            "valu": _gpu(b, factor_mfma=0, **opts)}


def test_inputs_are_the_ics_of_the_stated_ids(golden):
    """The shipped inputs are data_generation_ics(3, 4j .. 4j+3, N) of each horizon (to rounding of this host's
    numpy: the test's inputs are the shipped ones)."""
    from vboc_amd.ics import data_generation_ics
    for j, N in enumerate(HORIZONS):
        p = data_generation_ics(3, np.arange(PER * j, PER * j + PER), N=N)
        m = slice(PER * j, PER * j + PER)
        np.testing.assert_allclose(golden["in_x_guess"][m, :N + 1], p["x_guess"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(golden["in_p"][m], p["p"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(golden["in_lbx0"][m], p["lbx0"], rtol=0, atol=1e-12)


def test_ragged_horizons_bit_for_bit_against_the_parent(runs, golden):
    g = runs["mfma"]
    for j, N in enumerate(HORIZONS):
        m = slice(PER * j, PER * j + PER)
        print(f"N={N}: status {g['status'][m]} parent {golden['out_status'][m]} sqp {g['sqp_iter'][m]} parent "
              f"{golden['out_sqp_iter'][m]} qp {g['qp_iter'][m]} parent {golden['out_qp_iter'][m]} "
              f"max |dcost| {np.nanmax(np.abs(g['cost'][m] - golden['out_cost'][m])):.2e}")
    for k in ("status", "sqp_iter", "qp_iter", "cost"):
        np.testing.assert_array_equal(g[k], golden["out_" + k], err_msg=k)
    np.testing.assert_array_equal(g["x"][:, 0, :], golden["out_x0"], err_msg="x0")
    assert _sha1(g["x"]) == str(golden["out_x_sha1"]), "x"
    assert _sha1(g["u"]) == str(golden["out_u_sha1"]), "u"


def test_ragged_horizons_against_the_valu_factorisation(runs):
    """test_factor_solve.py's bars (tests/test_gpu.py's stated ones) against factor_mfma = 0."""
    g, r, b = runs["mfma"], runs["valu"], runs["b"]
    both = (g["status"] == 0) & (r["status"] == 0)
    dc_all = np.abs(g["cost"] - r["cost"])
    dx_all = np.abs(g["x"][:, 0, :6] - r["x"][:, 0, :6]).max(axis=1)
    for j, N in enumerate(HORIZONS):
        m = slice(PER * j, PER * j + PER)
        bb = both[m]
        print(f"mfma vs valu N={N}: status {g['status'][m]} / {r['status'][m]} sqp {g['sqp_iter'][m]} / "
              f"{r['sqp_iter'][m]} converged on both {bb.sum()}/{PER} "
              f"max dcost {dc_all[m][bb].max() if bb.any() else 0:.2e} max dx0 {dx_all[m][bb].max() if bb.any() else 0:.2e}")
    dc, dx = dc_all[both], dx_all[both]
    print(f"mfma vs valu: status agree {np.mean(g['status'] == r['status']):.4f} sqp agree "
          f"{np.mean(g['sqp_iter'] == r['sqp_iter']):.4f} both {both.sum()}/{len(both)} dcost median {np.median(dc):.2e} "
          f"max {dc.max():.2e} dx0 median {np.median(dx):.2e} max {dx.max():.2e}")
    assert np.mean(g["status"] == r["status"]) >= 0.98, (g["status"], r["status"])
    assert np.mean(g["sqp_iter"] == r["sqp_iter"]) >= 0.95, (g["sqp_iter"], r["sqp_iter"])
    assert both.sum() >= 0.5 * len(both)
    assert np.median(dc) <= 1e-9 and dc.max() <= 2e-3, (np.median(dc), dc.max())
    assert np.median(dx) <= 1e-9 and dx.max() <= 2e-3, (np.median(dx), dx.max())
    for i in np.where(both)[0]:
        N = b["N"][i]
        np.testing.assert_array_equal(g["x"][i, :N + 1, 6], b["lbx"][i, 6])


def test_ragged_horizons_twice_bit_equal(runs):
    for k in OUT_KEYS:
        np.testing.assert_array_equal(runs["mfma"][k], runs["again"][k], err_msg=k)


def test_device_loops_bit_for_bit_against_the_parent(golden):
    """k_dg<3, true> and k_ts<3, true> run the LDS-row passes: their rows and per-problem counts (solves, twin steps,
    SQP iterations) equal the parent's."""
    import sys
    from vboc_amd import lib
    sys.path.insert(0, os.path.join(lib.ROOT, "tools"))
    import record_lds_vectors as rec
    got = rec.device_loops()
    for k in ("dg_cnt", "dg_counts", "dg_rows", "ts_cnt", "ts_counts", "ts_rows"):
        print(k, got[k].shape, "parent", golden[k].shape)
        np.testing.assert_array_equal(got[k], golden[k], err_msg=k)
    assert (golden["dg_cnt"] > 0).sum() >= len(golden["dg_cnt"]) // 2   # the comparison is of real rows


def _loops_equal(got, golden, tag):
    keys = [f"{d}{tag}_{k}" for d in ("dg", "ts") for k in ("cnt", "counts", "rows")]
    for k in keys:
        print(k, got[k].shape, "parent", golden[k].shape)
    print(f"start {tag}: dg rows per problem {got[f'dg{tag}_cnt'].tolist()} solves {got[f'dg{tag}_counts'][:, 0].tolist()} "
          f"| ts rows {got[f'ts{tag}_cnt'].tolist()} solves {got[f'ts{tag}_counts'][:, 0].tolist()}")
    for k in keys:
        np.testing.assert_array_equal(got[k], golden[k], err_msg=k)


def _recorder():
    import sys
    from vboc_amd import lib
    sys.path.insert(0, os.path.join(lib.ROOT, "tools"))
    import record_lds_vectors as rec
    return rec


@pytest.mark.parametrize("start", [2, 3, 5, 51, 63, 108])
def test_device_loops_from_short_and_long_starts_against_the_parent(golden, start):
    """k_dg<3, true> and k_ts<3, true> started at `start` on Solver(3, 120): solves at start .. start + 12, so the
    LDS-row passes run the partial-group (2, 3), one- and two-group (4 .. 8), full-trip (63), one-lane-spill (64) and
    top-row (119, 120) horizons of the ragged batch.  Rows and per-problem counts equal the parent's."""
    rec = _recorder()
    assert start in rec.DG_STARTS
    got = rec.start_loops(start)
    _loops_equal(got, golden, str(start))
    assert (golden[f"dg{start}_counts"][:, 0] >= 1).all() and (golden[f"ts{start}_counts"][:, 0] >= 1).all()   # every problem solved


def test_device_loops_on_one_workgroup_against_the_parent(golden):
    """One workgroup takes the problems of both loops one after the other (start 108: horizons up to 120): whatever the
    longer solves - failed ones included - leave in the staging rows, their k_f words and the slack rows must not
    reach the next problem's first solves at N = 108, whose top groups load rows 108 .. 110."""
    rec = _recorder()
    got = rec.one_workgroup_loops()
    assert int(got["dg1_groups"]) == 1
    _loops_equal(got, golden, "1")
    assert (golden["dg1_counts"][:, 0] >= 2).all()   # every problem went past its first solve


def test_poisoned_rows_do_not_reach_later_problems(golden):
    """Problems with a control guess of 1e160 and N = 120 (the QP fails on non-finite values: the ring slots and the
    staging rows keep NaN / Inf words) share one workgroup (wave_groups = 1: one wave takes every job) with ordinary
    N = 100 problems, whose top groups load records past their last stage.  Whatever the job order, at least one
    poisoned problem is followed by ordinary ones; those equal a run without it, bit for bit.  This is the wave
    solver's kernel, which keeps the parent's passes (see Reach above)."""
    sel = np.array([44, 36, 37, 38, 32, 33, 45, 34, 35, 39])   # N = 120, 112 x3, 100 x2, 120, 100 x2, 112
    pois = (0, 6)
    keep = np.array([i for i in range(len(sel)) if i not in pois])
    b = {k: np.array(golden["in_" + k][sel], copy=True) for k in IN_KEYS}
    assert b["N"][list(pois)].tolist() == [120, 120] and (b["N"][keep] < 120).all() and (b["N"][keep] == 100).sum() == 4
    bp = {k: np.array(v, copy=True) for k, v in b.items()}
    for i in pois:
        bp["u_guess"][i] = 1e160
    opts = dict(slots=64, nlp_solver_max_iter=MAX_ITER, coop_threshold=8192, wave_all=1, wave_groups=1)
    clean, dirty = _gpu(b, **opts), _gpu(bp, **opts)
    assert clean["last_groups"] == 1 and dirty["last_groups"] == 1
    print("poisoned status", dirty["status"][list(pois)], "others", dirty["status"][keep], "clean", clean["status"])
    assert (dirty["status"][list(pois)] != 0).all(), dirty["status"]
    assert (clean["status"][keep] == 0).sum() >= len(keep) // 2
    for k in OUT_KEYS:
        np.testing.assert_array_equal(dirty[k][keep], clean[k][keep], err_msg=k)
