"""The oracle's own rounding spread on truncated solves of the free-time and Safe-MPC OCPs (oracle/vboc_oracle_ft.c):
the source of every tolerance of tests/test_truncated_parity_ft.py.  CPU only.  The method is tools/trunc_spread.py's
(its VARIANTS, copy-and-build loop, deviation and JSON writer are used from there): the oracle built with four
compiler-flag sets, every build run in a child process on every group and cut below, and per group and cut written to
tests/golden/trunc_spread_ft.json:

  * the ids, and per problem the committed build's status, sqp_iter and qp_iter;
  * spread: the max over builds and retained problems of max(|dx|, |du|) against the committed build, rows 0..N;
  * spread_cost: the same for |dcost| (absolute);
  * spread_h (Safe-MPC families): the same for |dh|, h the row at the result's x_N.

No trajectory and no weight is stored.  A problem whose counters differ between builds at any cut is dropped from its
group and listed; at most DROP_CAP per group, else the tool fails: choose other ids, do not raise the cap.

The tolerance rule (tol()): for a family, a cut and a quantity, TOL_FACTOR x the family's largest recorded spread of that
quantity at that cut over its groups.  Nothing measured on a GPU enters it.

Both sides stop in the same order (finiteness, RTI, convergence, it >= max_iter -> status 2, QP), so a cut
(m, q) = (nlp_solver_max_iter, qp_solver_iter_max) means the same thing to fsqp() and to ft.h run(); the cut (0, 1)
returns the guess with status 2, its cost and row evaluated.

Inputs are the same bits on every host: the pendulum's free-time law is vboc_amd.ics.pendulum_free_time_ics (Philox), every
other state and every network weight comes from np.random.default_rng(seed).uniform in float64 (no torch initialisation).

Families and groups (PER = 8 problems each):
  ft1       free-time pendulum, N in {1, 2, 3, 63, 64, 65, 130}: 63 puts one stage on every lane of the kernel's wave,
            64 and 65 are the first wrap of its `k = t; k <= N; k += 64` loops, 130 the third trip, 1 has no interior stage
  ft2, ft3  free-time double / triple, N in {2, 64, 65}: stage 0 with the positions pinned at a uniform point of the box
            (0.05 inside) and the velocities and dt free (nf0 = nq + 1), terminal velocities 0 with positions and dt boxed
            (ne = nq); guess: constant position, velocity 2 d for a unit direction d, dt 5e-3, u = 0; p = [-d, 1];
            dt in [0, 1e-2], the system's boxes
  ft3       N = 3 in three structure variants: free0 (every stage-0 component free, no terminal equality: nf0 = NX,
            ne = 0), fixN (x_0 pinned except dt, all 2 nq terminal states fixed: ne = 2 nq), freev (infinite velocity
            path bounds: free components)
  mpc-rti, mpc-sqp    the Safe-MPC OCP with the hard terminal row, (N, hid) in {(1, 1), (2, 63), (37, 500), (64, 64),
            (65, 65), (65, 512)} and (65, 0) without a row; MpcSpec(4e-3, 4e-3 N + 1e-9), mean pi, std 0.5
  soft-rti, soft-sqp  the soft rows, margin 5, the same six (N, hid), two weightings: `term` (Zl = 1e6 at stage N, 0
            elsewhere) and `all` (Zl = 1e4 on every stage, per-problem W [B, 9] and We [B, 6] that differ between problems)

usage: python tools/trunc_spread_ft.py [--out FILE]   (regenerates the fixture; the discrete counters must not change)
       python tools/trunc_spread_ft.py --scan         (per group, the ids of the pool whose counters no build changes)
"""
import os
import shutil
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trunc_spread as ts  # noqa: E402

ROOT = ts.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "trunc_spread_ft.json")

CUTS = ((0, 1),) + ts.CUTS
RTI_CUTS = ((0, 1), (1, 1), (1, 2), (1, 5), (1, 100))     # a later SQP cut is the same solve
PER, DROP_CAP, TOL_FACTOR = ts.PER, ts.DROP_CAP, ts.TOL_FACTOR
COUNTERS = ("status", "sqp_iter", "qp_iter")
FAMILIES = ("ft1", "ft2", "ft3", "mpc-rti", "mpc-sqp", "soft-rti", "soft-sqp")

FT_HORIZONS = {1: (1, 2, 3, 63, 64, 65, 130), 2: (2, 64, 65), 3: (2, 64, 65)}
FT_NMAX = 130
FT_VARIANTS = ("law", "free0", "fixN", "freev")
MPC_SHAPES = ((1, 1), (2, 63), (37, 500), (64, 64), (65, 65), (65, 512))
MEAN, STD = np.pi, 0.5
MARGIN = 5.0
SOFT_WEIGHTS = ("term", "all")

# Besides the four flag sets, two builds of the committed flags whose line search accepts a step at a merit of
# phi0 (1 +- 1e-15) instead of phi0 (oracle/vboc_oracle_ft.c VBOC_FT_LS_EPS).  A soft-row SQP often converges in x, u within
# two or three iterations while its multipliers lag; from then on the step is ~0, merit(alpha) equals merit(0) to rounding,
# and `pa < phi0` decides between alpha = 1 (multipliers jump, status 0) and alpha_min (nothing moves, status 2).  Flag sets
# flip few of these coins, so a problem whose counters change under either margin is dropped as build-dependent too.
LS_VARIANTS = (("ls_plus", ts.BASE + " -DVBOC_FT_LS_EPS=1e-15"), ("ls_minus", ts.BASE + " -DVBOC_FT_LS_EPS=-1e-15"))

# Groups whose ids are not the first PER of their generator's pool: the first PER ids that --scan lists as stable.  At
# N <= 2 (and in fixN) the SQP converges in x, u within a few iterations, and what follows is the rounding-decided line
# search above, or a QP that fails at an iteration count that depends on the flags.
IDS = {"ft3/N3/fixN": (0, 1, 3, 4, 5, 6, 7, 9),
       "mpc-rti/N2/h63": (0, 1, 3, 4, 5, 6, 7, 8),
       "mpc-sqp/N1/h1": (0, 2, 3, 4, 5, 6, 7, 8),
       "mpc-sqp/N2/h63": (0, 1, 4, 5, 7, 8, 9, 11),
       "soft-sqp/N1/h1/term": (2, 4, 5, 7, 8, 9, 10, 12),
       "soft-sqp/N1/h1/all": (2, 4, 5, 7, 8, 9, 10, 11),
       "soft-sqp/N2/h63/term": (1, 2, 4, 7, 8, 9, 11, 12),
       "soft-sqp/N2/h63/all": (0, 1, 2, 4, 5, 6, 7, 8)}
FT1_INFEASIBLE = (1, 2, 3)
POOL = 32     # every generator draws this many problems; a group's ids select among them


def group_key(g):
    if g["kind"] == "ft":
        return f"{g['family']}/N{g['N']}" + ("" if g["variant"] == "law" else f"/{g['variant']}")
    return f"{g['family']}/N{g['N']}/h{g['hid']}" + (f"/{g['weights']}" if g["kind"] == "soft" else "")


cut_key = ts.cut_key


def groups():
    """Every group: dict(family, kind, nq, N, ids, ...); ft: variant; mpc / soft: hid, rti; soft: weights."""
    out = []
    for j, N in enumerate(FT_HORIZONS[1]):     # the pendulum law's ids: consecutive blocks, like trunc_spread.groups()
        out.append(dict(family="ft1", kind="ft", nq=1, N=N, variant="law", ids=list(range(PER * j, PER * j + PER))))
    for nq in (2, 3):
        out += [dict(family=f"ft{nq}", kind="ft", nq=nq, N=N, variant="law", ids=list(range(PER)))
                for N in FT_HORIZONS[nq]]
    out += [dict(family="ft3", kind="ft", nq=3, N=3, variant=v, ids=list(range(PER))) for v in FT_VARIANTS[1:]]
    for rti in (True, False):
        fam = "mpc-rti" if rti else "mpc-sqp"
        out += [dict(family=fam, kind="mpc", nq=3, N=N, hid=hid, rti=rti, ids=list(range(PER)))
                for N, hid in MPC_SHAPES + ((65, 0),)]
    for rti in (True, False):
        fam = "soft-rti" if rti else "soft-sqp"
        out += [dict(family=fam, kind="soft", nq=3, N=N, hid=hid, rti=rti, weights=w, ids=list(range(PER)))
                for N, hid in MPC_SHAPES for w in SOFT_WEIGHTS]
    for g in out:
        g["ids"] = list(IDS.get(group_key(g), g["ids"]))
        if os.environ.get("TRUNC_SPREAD_FT_SCAN") and g["family"] != "ft1":
            g["ids"] = list(range(POOL))
    return out


def cuts_of(g):
    if g["family"] == "ft1" and g["N"] in FT1_INFEASIBLE:
        return tuple(c for c in CUTS if c[1] < 100)
    return RTI_CUTS if g.get("rti") else CUTS


# ------------------------------------------------------------------------------------------------ inputs
def ft_chain_batch(nq, N, ids, variant="law"):
    """The free-time OCPs of the double / triple (module docstring) in the vboc_amd.ics layout, nmax = N."""
    from vboc_amd.systems import system
    sd = system(nq)
    ids = np.asarray(ids)
    B, M, nx = ids.shape[0], POOL, 2 * nq + 1
    assert ids.max() < POOL
    rng = np.random.default_rng([1, nq, N, FT_VARIANTS.index(variant)])
    q0 = rng.uniform(sd.q_min + 0.05, sd.q_max - 0.05, (M, nq))[ids]
    v = rng.uniform(-1.0, 1.0, (M, nq))[ids]
    d = v / np.sqrt((v * v).sum(axis=1))[:, None]
    lbx = np.tile(np.r_[[sd.q_min] * nq, [-sd.v_max] * nq, 0.0], (B, 1))
    ubx = np.tile(np.r_[[sd.q_max] * nq, [sd.v_max] * nq, 1e-2], (B, 1))
    lbx0, ubx0, lbxe, ubxe = lbx.copy(), ubx.copy(), lbx.copy(), ubx.copy()
    if variant in ("law", "freev"):
        lbx0[:, :nq] = ubx0[:, :nq] = q0
        lbxe[:, nq:2 * nq] = ubxe[:, nq:2 * nq] = 0.0
    elif variant == "fixN":
        lbx0[:, :nq] = ubx0[:, :nq] = q0
        lbx0[:, nq:2 * nq] = ubx0[:, nq:2 * nq] = 0.2 * d
        lbxe[:, :nq] = ubxe[:, :nq] = q0 + 0.003 * d
        lbxe[:, nq:2 * nq] = ubxe[:, nq:2 * nq] = 0.0
    if variant == "freev":
        lbx[:, nq:2 * nq], ubx[:, nq:2 * nq] = -np.inf, np.inf
    xg = np.zeros((B, N + 1, nx))
    xg[:, :, :nq], xg[:, :, nq:2 * nq], xg[:, :, 2 * nq] = q0[:, None], 2.0 * d[:, None], 5e-3
    return dict(N=np.full(B, N, np.int32), x_guess=xg, u_guess=np.zeros((B, N, nq)), p=np.c_[-d, np.ones(B)],
                lbx=lbx, ubx=ubx, lbu=np.full((B, nq), -sd.u_max), ubu=np.full((B, nq), sd.u_max),
                lbx0=lbx0, ubx0=ubx0, lbxe=lbxe, ubxe=ubxe)


def mpc_inputs(N, hid, ids):
    """Safe-MPC states, guesses, network and per-problem weights of the (N, hid) groups: dict(spec, x0, xg, ug, params
    (None for hid 0), W, We).  One generator per (N, hid), drawn in a fixed order."""
    from vboc_amd.safempc import MpcSpec
    sp = MpcSpec(4e-3, 4e-3 * N + 1e-9)
    assert sp.N == N
    ids = np.asarray(ids)
    B, M = ids.shape[0], POOL
    assert ids.max() < POOL
    rng = np.random.default_rng([2, N, hid])
    x0 = np.zeros((B, 6))
    x0[:, :3] = rng.uniform(sp.thetamin, sp.thetamax, (M, 3))[ids]
    x0[:, 3:] = rng.uniform(-2.0, 2.0, (M, 3))[ids]
    q0 = (1e-2 + 10.0 ** rng.uniform(0.0, 2.0, M))[ids]
    W = np.tile(sp.W, (B, 1))
    W[:, 0] = q0
    params = None
    if hid > 0:      # float64 weights, +-1 / sqrt(fan_in); output bias 4.0 so the row is in play
        u = lambda shape, fan: rng.uniform(-1.0, 1.0, shape) / np.sqrt(float(fan))
        params = [u((hid, 6), 6), u((hid,), 6), u((hid, hid), hid), u((hid,), hid), u((1, hid), hid), np.array([4.0])]
    return dict(spec=sp, x0=x0, xg=np.repeat(x0[:, None, :], N + 1, 1), ug=np.zeros((B, N, 3)), params=params,
                W=W, We=W[:, :6].copy())


def soft_Zl(N, weights):
    Zl = np.zeros(N + 1)
    if weights == "term":
        Zl[N] = 1e6
    else:
        Zl[:] = 1e4
    return Zl


def batch(g):
    """The group's inputs: the vboc_amd.ics layout (ft) or mpc_inputs() (mpc, soft)."""
    if g["kind"] != "ft":
        return mpc_inputs(g["N"], g["hid"], g["ids"])
    if g["nq"] == 1:
        from vboc_amd.ics import pendulum_free_time_ics
        b = pendulum_free_time_ics(np.asarray(g["ids"]), (g["N"], g["N"]))
        return {k: b[k] for k in ts.KEYS}
    return ft_chain_batch(g["nq"], g["N"], g["ids"], g["variant"])


def mpc_opts(oracle, sp, cut, **kw):
    return oracle.default_opts(lm=sp.lm, tol_stat=1e-6, qp_tol_stat=1e-8, max_iter=cut[0], qp_max_iter=cut[1], **kw)


def oracle_solve(oracle, g, b, cut, **kw):
    """dict(status, sqp_iter, qp_iter, cost, x, u[, h]) of the loaded oracle library on the group at the cut; kw: further
    vboc_opts_t fields."""
    n = len(g["ids"])
    if g["kind"] == "ft":
        o = oracle.default_opts(max_iter=cut[0], qp_max_iter=cut[1], **kw)
        x, u, r = oracle.solve_batch(g["nq"], *[b[k] for k in ts.KEYS], opts=o, nthreads=n, free_time=True)
        h = None
    elif g["kind"] == "mpc":
        x, u, r, h = oracle.mpc_solve_batch(b["spec"], b["x0"], b["xg"], b["ug"], b["params"], mean=MEAN, std=STD,
                                            rti=g["rti"], opts=mpc_opts(oracle, b["spec"], cut, **kw), nthreads=n)
    else:
        per = g["weights"] == "all"
        x, u, r, h = oracle.mpc_soft_solve_batch(b["spec"], b["x0"], b["xg"], b["ug"], b["params"], MEAN, STD, MARGIN,
                                                 soft_Zl(g["N"], g["weights"]), W=b["W"] if per else None,
                                                 We=b["We"] if per else None, rti=g["rti"],
                                                 opts=mpc_opts(oracle, b["spec"], cut, **kw), nthreads=n)
    out = dict(status=np.array(r["status"]), sqp_iter=np.array(r["sqp_iter"]), qp_iter=np.array(r["qp_iter"]),
               cost=np.array(r["cost"]), x=x, u=u)
    if h is not None:
        out["h"] = h
    return out


deviation = ts.deviation


def solved(r):
    """The problems whose structure the solver accepts (status 5: no iterate is returned, only the counters compare)."""
    return r["status"] != 5


def tol(fixture, family, cut, what="spread"):
    """TOL_FACTOR x the largest recorded spread of the quantity in the family at the cut over its groups."""
    s = [e["cuts"][cut_key(cut)][what] for e in fixture["groups"].values()
         if e["family"] == family and cut_key(cut) in e["cuts"]]
    return TOL_FACTOR * max(s)


def _child(out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    import oracle
    assert os.environ.get("VBOC_ORACLE_LIB") and oracle.LIB == os.environ["VBOC_ORACLE_LIB"]
    save = {}
    for g in groups():
        b = batch(g)
        for cut in cuts_of(g):
            for k, v in oracle_solve(oracle, g, b, cut).items():
                save[f"{group_key(g)}|{cut_key(cut)}|{k}"] = v
    np.savez(out, **save)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return _child(sys.argv[2])
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    scan = "--scan" in sys.argv
    if scan:
        os.environ["TRUNC_SPREAD_FT_SCAN"] = "1"
    tmp = tempfile.mkdtemp(prefix="trunc_spread_ft_")
    try:
        runs, skipped = ts.run_variants(tmp, __file__, ts.VARIANTS + LS_VARIANTS)
        ls = {n: runs.pop(n) for n, _ in LS_VARIANTS}     # for the drop rule only: no spread is taken from them
        base = runs["committed"]
        if scan:
            for g in groups():
                get = lambda run, cut, k: run[f"{group_key(g)}|{cut_key(cut)}|{k}"]
                keep = np.ones(len(g["ids"]), bool)
                for cut in cuts_of(g):
                    for run in list(runs.values()) + list(ls.values()):
                        for k in COUNTERS:
                            keep &= get(run, cut, k) == get(base, cut, k)
                print(group_key(g), [i for i, ok in zip(g["ids"], keep) if ok])
            return
        fx = dict(cuts=[list(c) for c in CUTS], rti_cuts=[list(c) for c in RTI_CUTS], tol_factor=TOL_FACTOR,
                  drop_cap=DROP_CAP, variants={n: f for n, f in ts.VARIANTS if n in runs}, skipped_variants=skipped,
                  line_search_variants=dict(LS_VARIANTS), groups={})
        over = []
        for g in groups():
            B, key = len(g["ids"]), group_key(g)
            get = lambda run, cut, k: run[f"{key}|{cut_key(cut)}|{k}"]
            keep = np.ones(B, bool)
            for cut in cuts_of(g):
                for run in list(runs.values()) + list(ls.values()):
                    for k in COUNTERS:
                        keep &= get(run, cut, k) == get(base, cut, k)
            dropped = [g["ids"][i] for i in np.where(~keep)[0]]
            if len(dropped) > DROP_CAP:
                over.append(f"{key}: {len(dropped)} problems with counters that depend on the build ({dropped})")
                continue
            e = dict(g, dropped=dropped, cuts={})
            for cut in cuts_of(g):
                a = {k: get(base, cut, k) for k in ("status", "x", "u", "cost") + (("h",) if g["kind"] != "ft" else ())}
                m = keep & solved(a)
                spread = dict(spread=0.0, spread_cost=0.0)
                if "h" in a:
                    spread["spread_h"] = 0.0
                for run in runs.values():
                    if not m.any():
                        break
                    assert np.array_equal(np.isnan(get(run, cut, "cost"))[m], np.isnan(a["cost"])[m]), (key, cut)
                    d = deviation(g, a, {k: get(run, cut, k) for k in ("x", "u")})
                    spread["spread"] = max(spread["spread"], float(d[m].max()))
                    dc = np.abs(get(run, cut, "cost") - a["cost"])[m]
                    spread["spread_cost"] = max(spread["spread_cost"], float(np.nanmax(dc)))
                    if "h" in a:
                        spread["spread_h"] = max(spread["spread_h"], float(np.abs(get(run, cut, "h") - a["h"])[m].max()))
                e["cuts"][cut_key(cut)] = dict({k: get(base, cut, k).tolist() for k in COUNTERS}, **spread)
            fx["groups"][key] = e
        if over:
            raise RuntimeError("\n".join(over) + "\nchoose other ids (--scan lists the stable ones of the pool)")
        ts.write_fixture(out, fx)
        for what in ("spread", "spread_cost", "spread_h"):
            for fam in FAMILIES[3 if what == "spread_h" else 0:]:
                cuts = RTI_CUTS if fam.endswith("rti") else CUTS
                print(f"{what:12s} {fam:9s}", " ".join(f"{tol(fx, fam, c, what) / TOL_FACTOR:.1e}" for c in cuts))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
