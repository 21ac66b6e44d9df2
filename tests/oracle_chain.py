"""The CPU oracle's tracking-OCP entry points for any pendulum chain (test helper).

oracle/oracle.py binds vboc_oracle_mpc_solve_batch, vboc_oracle_mpc_soft_solve_batch, vboc_oracle_al_solve_batch and
vboc_oracle_mpc_row with the triple's widths (nq = 3, shapes 6 / 3 / 9); the C functions themselves take nq and accept
1 <= nq <= 3 (oracle/vboc_oracle_ft.c).  These wrappers call the same functions with the spec's nq.  A per-problem
reference (the 2dof classes' OCP_solve(x0, q_ref, ...)) is a loop over vboc_oracle_mpc_solve / _mpc_solve_soft, whose
yref is per call.

Also here: the nq-generic form of tests/al_reference.py's independent LP pin of the AL labels."""
import ctypes
import os

import numpy as np
import scipy.sparse as sp
from scipy.optimize import linprog

import oracle
from oracle import RESULT_DTYPE, MpcNN, _mpc_nn, _p, default_opts


class MpcSoft(ctypes.Structure):
    """vboc_mpc_soft_t (oracle/vboc_oracle.h): the soft rows of one problem."""
    _fields_ = [("margin", ctypes.c_double), ("zl", ctypes.c_void_p), ("Zl", ctypes.c_void_p)]


def mpc_opts(spec, **kw):
    """The oracle's options for a Safe-MPC spec: the triple's class sets no tolerance (ACADOS' 1e-6), the double's
    sets tol = 1e-2 on the four NLP tolerances."""
    if getattr(spec, "tol", None) is not None:
        o = dict(lm=spec.lm, tol_stat=spec.tol, tol_eq=spec.tol, tol_ineq=spec.tol, tol_comp=spec.tol,
                 qp_tol_stat=1e-8, qp_max_iter=spec.qp_iter_max, max_iter=spec.max_iter)
    else:
        o = dict(lm=spec.lm, tol_stat=1e-6, qp_tol_stat=1e-8)
    o.update(kw)
    return default_opts(**o)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def al_solve_batch(spec, x0, x_guess=None, opts=None, nthreads=None):
    """oracle.al_solve_batch for spec.nq: dict(label, status, qp_iter, x [B, N+1, 2nq], u [B, N, nq])."""
    nq = spec.nq
    x0 = _f64(x0)
    B, N = x0.shape[0], spec.N
    assert x0.shape == (B, 2 * nq)
    xg = None if x_guess is None else _f64(x_guess)
    assert xg is None or xg.shape == (B, N + 1, 2 * nq)
    x_out, u_out = np.zeros((B, N + 1, 2 * nq)), np.zeros((B, N, nq))
    res = np.zeros(B, dtype=RESULT_DTYPE)
    label = np.zeros(B, np.int32)
    if opts is None:
        opts = default_opts(lm=spec.lm, tol_stat=1e-6, qp_tol_stat=1e-8, qp_max_iter=spec.qp_iter_max)
    vec = [_f64(a) for a in (spec.xmin, spec.xmax, spec.umin, spec.umax, spec.xmin_e, spec.xmax_e, spec.W, spec.W_e)]
    rc = oracle.lib().vboc_oracle_al_solve_batch(nq, B, N, ctypes.c_double(spec.time_step), _p(x0),
                                                 _p(xg) if xg is not None else None, *[_p(a) for a in vec],
                                                 ctypes.c_double(spec.cost_scale), ctypes.byref(opts),
                                                 int(nthreads or os.cpu_count()), _p(x_out), _p(u_out), _p(res),
                                                 _p(label))
    if rc != 0:
        raise RuntimeError(f"oracle al_solve_batch failed rc={rc}")
    return dict(label=label, status=np.array(res["status"]), qp_iter=np.array(res["qp_iter"]), x=x_out, u=u_out)


def mpc_solve_batch(spec, x0, x_guess, u_guess, params=None, mean=0.0, std=1.0, rti=False, opts=None, nthreads=None,
                    lh=0.0, uh=1e6, yref=None, yref_e=None, soft=None):
    """The Safe-MPC OCP_solve on the oracle for spec.nq.  yref [B, 3nq] / yref_e [B, 2nq]: per-problem references
    (None: the spec's).  soft: dict(margin, Zl [B, N+1], zl / W / We optional per-problem arrays) - the soft-row
    classes.  Every problem is one call of vboc_oracle_mpc_solve(_soft).  Returns (x, u, results, h(x_N))."""
    nq = spec.nq
    x0, xg, ug = _f64(x0), _f64(x_guess), _f64(u_guess)
    B, N = x0.shape[0], spec.N
    assert xg.shape == (B, N + 1, 2 * nq) and ug.shape == (B, N, nq)
    x_out, u_out = np.zeros_like(xg), np.zeros_like(ug)
    res = np.zeros(B, dtype=RESULT_DTYPE)
    hrow = np.zeros(B)
    if opts is None:
        opts = mpc_opts(spec)
    bnd = [_f64(a) for a in (spec.xmin, spec.xmax, spec.umin, spec.umax, spec.xmin, spec.xmax)]
    bc = lambda a, d, w: _f64(np.broadcast_to(np.asarray(d if a is None else a, dtype=np.float64), (B, w)))
    yr, yre = bc(yref, spec.yref, 3 * nq), bc(yref_e, spec.yref_e, 2 * nq)
    sf = soft or {}
    W, We = bc(sf.get("W"), spec.W, 3 * nq), bc(sf.get("We"), spec.W_e, 2 * nq)
    nnp, keep = (None, None) if params is None else _mpc_nn(params, mean, std, lh, uh)
    if soft is not None:
        Zl = bc(soft["Zl"], 0.0, N + 1)
        zl = bc(soft.get("zl"), 0.0, N + 1)
    L = oracle.lib()
    for b in range(B):
        common = (nq, N, ctypes.c_double(spec.time_step), _p(x0[b]), _p(xg[b]), _p(ug[b]), *[_p(a) for a in bnd],
                  _p(W[b]), _p(We[b]), _p(yr[b]), _p(yre[b]), ctypes.c_double(spec.cost_scale),
                  ctypes.byref(nnp) if nnp is not None else None)
        tail = (int(bool(rti)), ctypes.byref(opts), _p(x_out[b]), _p(u_out[b]), _p(res[b:b + 1]), _p(hrow[b:b + 1]))
        if soft is not None:
            s_ = MpcSoft(margin=float(soft["margin"]), zl=zl[b].ctypes.data, Zl=Zl[b].ctypes.data)
            rc = L.vboc_oracle_mpc_solve_soft(*common, ctypes.byref(s_), *tail)
        else:
            rc = L.vboc_oracle_mpc_solve(*common, *tail)
        if rc == -2:
            res[b]["status"], res[b]["cost"] = 5, np.nan
        elif rc != 0:
            raise RuntimeError(f"oracle mpc_solve failed rc={rc}")
    del keep
    return x_out, u_out, res, hrow


def mpc_row(nq, x, params, mean, std, margin=-1.0):
    """The Safe-MPC row at states x [B, 2nq] (vboc_oracle_mpc_row): margin >= 0 the margin-scaled (soft) row."""
    x = _f64(np.atleast_2d(x))
    assert x.shape[1] == 2 * nq
    out = np.zeros(x.shape[0])
    nnp, keep = _mpc_nn(params, mean, std)
    oracle.lib().vboc_oracle_mpc_row(nq, x.shape[0], _p(x), ctypes.byref(nnp), ctypes.c_double(float(margin)), _p(out))
    del keep
    return out


def forced_failure(x0, Zl, fail_mod):
    """Deterministic failure injection for the closed loops (as tests/oracle_backend.py forced_failure: the drivers'
    failure branches are rarely reached by the solver on its own): a solve reports status 4 when
    int(|x0[0]| 200) + 7 (stage of the largest Zl) is divisible by fail_mod.  Keyed on the request alone - the state,
    in bins of 5e-3 rad that a closed loop crosses in one to a few dozen steps, so failures come in runs of every
    length around the drivers' N - 1 limit, and, for the parallel driver's candidates, the placement of the stiff slack
    weight - so every solver that is asked the same question fails the same way."""
    if fail_mod <= 0:
        return False
    k = 0 if Zl is None else int(np.argmax(Zl))
    return (int(abs(float(x0[0])) * 200) + 7 * k) % fail_mod == 0


def with_forced_failures(solve, fail_mod, Zl_default=None):
    """solve(x0, xg, ug[, weights]) with forced_failure applied to its statuses; Zl_default: the slack weights of a
    solve that is passed none (the soft_traj driver's, set once with cost_set)."""
    def wrapped(x0, xg, ug, w=None):
        r = dict(solve(x0, xg, ug, w) if w is not None else solve(x0, xg, ug))
        st = np.array(r["status"], copy=True)
        for j in range(st.shape[0]):
            if forced_failure(x0[j], Zl_default if w is None or w.get("Zl") is None else w["Zl"][j], fail_mod):
                st[j] = 4
        r["status"] = st
        return r
    return wrapped


def rk4(nq, h):
    return lambda X, U: np.stack([oracle.rk4(nq, h, X[i], U[i]) for i in range(X.shape[0])])


# ----------------------------------------------------------------------------------------------------------------
# the independent LP pin of AL's labels (tests/al_reference.py), for any chain
# ----------------------------------------------------------------------------------------------------------------
def guesses(spec, x0, x_guess=None):
    nq = spec.nq
    xg = np.tile(np.r_[x0[:nq], np.zeros(nq)], (spec.N + 1, 1)) if x_guess is None else np.array(x_guess, dtype=float)
    xg[0] = x0
    return xg


def linearisation(spec, x0, x_guess=None):
    xg = guesses(spec, x0, x_guess)
    out = []
    for k in range(spec.N):
        x1, A, B = oracle.rk4_sens(spec.nq, spec.time_step, xg[k], np.zeros(spec.nq))
        out.append((A, B, x1 - xg[k + 1]))
    return out


def lp_feasible(spec, x0, x_guess=None):
    """True if the linearised QP of compute_problem(x0) has a feasible point (HiGHS on the zero-objective LP over
    du_0..du_{N-1}, dx_1..dx_N: the linearised dynamics, the path boxes, the terminal box with its fixed velocities)."""
    N, nq, nx = spec.N, spec.nq, 2 * spec.nq
    xgs = guesses(spec, x0, x_guess)
    nvar = nq * N + nx * N
    iu = lambda k: nq * k
    ix = lambda k: nq * N + nx * (k - 1)
    rows, cols, vals, beq = [], [], [], []
    r = 0
    for k, (A, B, b) in enumerate(linearisation(spec, x0, x_guess)):
        for i in range(nx):       # dx_{k+1} - A_k dx_k - B_k du_k = b_k  (dx_0 = 0: x_0 is fixed)
            rows.append(r); cols.append(ix(k + 1) + i); vals.append(1.0)
            if k > 0:
                for q in range(nx):
                    rows.append(r); cols.append(ix(k) + q); vals.append(-A[i, q])
            for a in range(nq):
                rows.append(r); cols.append(iu(k) + a); vals.append(-B[i, a])
            beq.append(b[i])
            r += 1
    Aeq = sp.csr_matrix((vals, (rows, cols)), shape=(r, nvar))
    lo, hi = np.empty(nvar), np.empty(nvar)
    for k in range(N):
        lo[iu(k):iu(k) + nq], hi[iu(k):iu(k) + nq] = spec.umin, spec.umax
    for k in range(1, N + 1):
        xl, xh = (spec.xmin_e, spec.xmax_e) if k == N else (spec.xmin, spec.xmax)
        lo[ix(k):ix(k) + nx], hi[ix(k):ix(k) + nx] = xl - xgs[k], xh - xgs[k]
    res = linprog(np.zeros(nvar), A_eq=Aeq, b_eq=np.array(beq), bounds=list(zip(lo, hi)), method="highs")
    assert res.status in (0, 2), res.message
    return res.status == 0


def step_violation(spec, x0, x, u, x_guess=None):
    """Largest violation, by the returned step, of the linearised QP's constraints: the linearised dynamics, x_0, the
    boxes, the terminal velocities."""
    xg = guesses(spec, x0, x_guess)
    v = float(np.abs(x[0] - x0).max())
    for k, (A, B, b) in enumerate(linearisation(spec, x0, x_guess)):
        v = max(v, float(np.abs(x[k + 1] - xg[k + 1] - (A @ (x[k] - xg[k]) + B @ u[k] + b)).max()))
    if spec.N > 1:
        v = max(v, float(np.max(np.r_[spec.xmin - x[1:-1].min(0), x[1:-1].max(0) - spec.xmax])))
    v = max(v, float(np.max(np.r_[spec.umin - u.min(0), u.max(0) - spec.umax])))
    v = max(v, float(np.max(np.r_[spec.xmin_e - x[-1], x[-1] - spec.xmax_e])))
    return v
