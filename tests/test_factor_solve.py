"""The triple's MFMA factorisation also runs the predictor's Riccati vector step (coop.h, VFUSE: one stage behind the
matrix recursion, on the ring slot of the stage it has just completed).  GPU tests of the shapes at which that sweep
can go wrong, at test_gpu.py's stated bars (status agreement >= 98 %, SQP-iteration agreement >= 95 %, problems
converged on both: median |dcost| and |dx0| <= 1e-9, max <= 2e-3):

  * horizons N = 2 (the only interior stage is finished by the sweep's tail), 3 (first trip through the loop's
    write-back), 4, 6, 7 (the 4-slot ring wraps), 9, 100 and 120 (the workload's horizons and nmax) in one ragged
    batch on the wave solver, against the oracle, against the same library with factor_mfma = 0 (the VALU
    factorisation and the separate vector passes) and against itself (bit-equal);
  * a problem that leaves non-finite values in the factorisation's ring slots, followed on the same workgroup region
    by ordinary problems: those must equal, bit for bit, a run without it.

Measured on MI355X, the same figures on the parent commit's library and on the fused one (the fused step is
bit-identical): against the oracle status and SQP-iteration agreement 128 / 128, 124 converged on both, |dcost| median
2.1e-12, max 4.7e-11, |dx0| median 1.7e-12, max 4.5e-11; against the VALU factorisation 128 / 128, |dcost| max 5.1e-11.
No horizon had to be dropped.  The poisoned problems end with status 4 (the QP fails on the non-finite factorisation),
not 1: a guess that fails the first linearisation's finiteness test never reaches the factorisation, so it could not
leave anything in the slots.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HORIZONS = (2, 3, 4, 6, 7, 9, 100, 120)
PER = 16
NMAX = 120
MAX_ITER = 200


def _ragged():
    from vboc_amd.ics import data_generation_ics
    parts = [data_generation_ics(3, np.arange(PER * j, PER * j + PER), N=N) for j, N in enumerate(HORIZONS)]
    b = {}
    for k in parts[0]:
        if k in ("joint_sel", "vel_sel"):
            continue
        arrs = []
        for p in parts:
            a = p[k]
            if k == "x_guess":
                a = np.concatenate([a, np.repeat(a[:, -1:], NMAX + 1 - a.shape[1], 1)], 1)
            if k == "u_guess":
                a = np.concatenate([a, np.zeros((a.shape[0], NMAX - a.shape[1], a.shape[2]))], 1)
            arrs.append(a)
        b[k] = np.concatenate(arrs)
    return b


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
def runs():
    import oracle
    b = _ragged()
    assert int(b["N"].max()) == NMAX and sorted(set(b["N"].tolist())) == sorted(HORIZONS)
    opts = dict(nlp_solver_max_iter=MAX_ITER, coop_threshold=8192, wave_all=1)
    xo, uo, r = oracle.solve_batch(3, b["N"], b["x_guess"], b["u_guess"], b["p"], b["lbx"], b["ubx"], b["lbu"],
                                   b["ubu"], b["lbx0"], b["ubx0"], b["lbxe"], b["ubxe"],
                                   opts=oracle.default_opts(max_iter=MAX_ITER))
    return {"b": b, "mfma": _gpu(b, factor_mfma=1, **opts), "again": _gpu(b, factor_mfma=1, **opts),
            "valu": _gpu(b, factor_mfma=0, **opts), "oracle": r, "oracle_x": xo}


def _bars(g, r, rx, b, what):
    """_compare's checks (tests/test_gpu.py) of one result set against another (r, its states rx), figures printed
    first."""
    both = (g["status"] == 0) & (r["status"] == 0)
    dc_all = np.abs(g["cost"] - r["cost"])
    dx_all = np.abs(g["x"][:, 0, :6] - rx[:, 0, :6]).max(axis=1)
    for j, N in enumerate(HORIZONS):
        m = slice(PER * j, PER * j + PER)
        bb = both[m]
        print(f"{what} N={N}: status agree {np.mean(g['status'][m] == r['status'][m]):.3f} "
              f"sqp agree {np.mean(g['sqp_iter'][m] == r['sqp_iter'][m]):.3f} converged on both {bb.sum()}/{PER} "
              f"max dcost {dc_all[m][bb].max() if bb.any() else 0:.2e} max dx0 {dx_all[m][bb].max() if bb.any() else 0:.2e}")
    dc, dx = dc_all[both], dx_all[both]
    print(f"{what}: status agree {np.mean(g['status'] == r['status']):.4f} sqp agree "
          f"{np.mean(g['sqp_iter'] == r['sqp_iter']):.4f} both {both.sum()}/{len(both)} dcost median {np.median(dc):.2e} "
          f"max {dc.max():.2e} dx0 median {np.median(dx):.2e} max {dx.max():.2e}")
    assert np.mean(g["status"] == r["status"]) >= 0.98, (g["status"], r["status"])
    assert np.mean(g["sqp_iter"] == r["sqp_iter"]) >= 0.95, (g["sqp_iter"], r["sqp_iter"])
    assert both.sum() >= 0.5 * len(both)
    assert np.median(dc) <= 1e-9 and dc.max() <= 2e-3, (np.median(dc), dc.max())
    assert np.median(dx) <= 1e-9 and dx.max() <= 2e-3, (np.median(dx), dx.max())
    for i in np.where(both)[0][:8]:
        N = b["N"][i]
        np.testing.assert_array_equal(g["x"][i, :N + 1, 6], b["lbx"][i, 6])


def test_short_and_ragged_horizons_against_the_oracle(runs):
    _bars(runs["mfma"], runs["oracle"], runs["oracle_x"], runs["b"], "mfma vs oracle")


def test_short_and_ragged_horizons_against_the_valu_factorisation(runs):
    _bars(runs["mfma"], runs["valu"], runs["valu"]["x"], runs["b"], "mfma vs valu")


def test_short_and_ragged_horizons_twice_bit_equal(runs):
    for k in ("status", "sqp_iter", "qp_iter", "cost", "x", "u"):
        np.testing.assert_array_equal(runs["mfma"][k], runs["again"][k], err_msg=k)


def test_poisoned_slot_does_not_reach_later_problems():
    """Problems whose factorisation meets non-finite values (a control guess of 1e160: the QP fails, K, Ru^-1 and
    P e of their stages are NaN in the ring slots and the window words are Inf) share one workgroup region with
    ordinary problems (wave_groups = 1: one wave takes every job).  Whatever the job order, at least one of the
    two is followed by ordinary problems; those equal a run without the poisoned ones, bit for bit."""
    from vboc_amd.ics import data_generation_ics
    B, POIS = 12, (0, 6)
    keep = np.array([i for i in range(B) if i not in POIS])
    b = {k: v for k, v in data_generation_ics(3, np.arange(B), N=100).items() if k not in ("joint_sel", "vel_sel")}
    bp = {k: np.array(v, copy=True) for k, v in b.items()}
    for i in POIS:
        bp["u_guess"][i] = 1e160
    opts = dict(slots=64, nlp_solver_max_iter=MAX_ITER, coop_threshold=8192, wave_all=1, wave_groups=1)
    clean, dirty = _gpu(b, **opts), _gpu(bp, **opts)
    assert clean["last_groups"] == 1 and dirty["last_groups"] == 1
    print("poisoned status", dirty["status"][list(POIS)], "others", dirty["status"][keep], "clean", clean["status"])
    assert (dirty["status"][list(POIS)] != 0).all(), dirty["status"]
    assert (clean["status"][keep] == 0).sum() >= len(keep) // 2
    for k in ("status", "sqp_iter", "qp_iter", "cost", "x", "u"):
        np.testing.assert_array_equal(dirty[k][keep], clean[k][keep], err_msg=k)
