"""Active learning's labelling OCP on the batched solver (AL/).

The reference (`AL/triplependulum_class_al.py`) labels a state x0 = (q0, v0) by ONE call of ACADOS on the OCP of
OCPtriplependulum (:82-144) with the terminal rest of OCPtriplependulumINIT (:204-222):
  model     the triple pendulum, nx 6 (no dt state), nu 3, ERK4 on tf = 1 over N = 100 intervals (:85-89)
  cost      LINEAR_LS 1/2 |[x; u]|^2_W, W = blockdiag(Q, R), Q = 2 diag(0, 0, 0, 1, 1, 1), R = 0; W_e = Q (:97-115)
  bounds    theta in [3pi/4, 5pi/4], |dtheta| <= 10, |C| <= 10 on the path and at N (:118-141); terminal
            velocities fixed to 0 (lbx_e = ubx_e = 0, :210-216)
  options   none set: ACADOS' defaults - SQP_RTI (ONE QP at the reset point and its full step), GAUSS_NEWTON,
            levenberg_marquardt 0, qp_solver_iter_max 50 (PARTIAL_CONDENSING_HPIPM)
  compute_problem(q0, v0) (:148-169): reset (u = 0, multipliers 0), x_0 fixed by lbx = ubx, every stage's x guess
            (q0, 0); returns 1 if the solve's status is 0, 0 if it is 4 (QP failure), 2 otherwise.
The single QP's feasibility is the label.  The restatement (oracle/vboc_oracle_ft.c vboc_oracle_al_solve_batch,
vboc_amd/csrc/ft.h through vboc_al_solve_batch) solves that QP with the Safe-MPC solver's interior-point method and
counts a QP the IPM has not finished after qp_solver_iter_max iterations as a failure (status 4); HPIPM's own
status on such a QP is unpinned (ACADOS / HPIPM are not in this image).  The tests pin the label against an
independent LP feasibility check of the same linearised QP (tests/test_al.py).  The driver `testing(s0)`
(AL/triplependulum_al.py:24-42) is `testing_batch` below; with the guess network (compute_problem_nnguess, :171-201) the
same function restates `testing_guess(s0)` (:44-62).
"""
import math

import numpy as np


class AlSpec:
    """The OCP data of the AL classes: nq 3 OCPtriplependulumINIT (AL/triplependulum_class_al.py:82-144, 204-222, the
    line numbers below), nq 2 OCPdoublependulumINIT (AL/doublependulum_class_al.py:118-186, 402-420: the same data on
    four states), nq 1 OCPpendulumINIT (AL/pendulum_class_al.py:62-125, 286-300: the damped pendulum, |F| <= Fmax = 3,
    SQP_RTI set explicitly).  AlSpec() is the triple's."""

    def __init__(self, nq=3, cost_scale=None):
        if nq not in (1, 2, 3):
            raise ValueError(f"AlSpec: nq = {nq} (the AL classes are the pendulum's, the double's and the triple's)")
        self.nq, self.nx, self.nu = nq, 2 * nq, nq
        self.Tf = 1.0                                   # :85
        self.N = int(100 * self.Tf)                     # :88
        self.time_step = self.Tf / self.N
        self.Cmax = 3.0 if nq == 1 else 10.0            # :118 (pendulum_class_al.py:100 Fmax = 3)
        self.Fmax = self.Cmax
        self.thetamax = math.pi / 4 + math.pi           # :119
        self.thetamin = -math.pi / 4 + math.pi          # :120
        self.dthetamax = 10.0                           # :121
        self.Q = 2.0 * np.array([0.0] * nq + [1.0] * nq)           # :98
        self.R = 2.0 * np.zeros(nq)                                # :99
        self.W = np.concatenate([self.Q, self.R])
        self.W_e = self.Q.copy()
        self.xmax = np.array([self.thetamax] * nq + [self.dthetamax] * nq)
        self.xmin = np.array([self.thetamin] * nq + [-self.dthetamax] * nq)
        self.umax = np.full(nq, self.Cmax)
        self.umin = -self.umax
        self.xmax_e, self.xmin_e = self.xmax.copy(), self.xmin.copy()
        self.xmax_e[nq:] = self.xmin_e[nq:] = 0.0       # :210-216 zero final velocity
        # ACADOS' cost_scaling: stage costs times the time step in current releases, 1 in older ones - unpinned; the
        # choice matters for the step's trajectory, not for the QP's feasibility (the label)
        self.cost_scale = self.time_step if cost_scale is None else float(cost_scale)
        self.lm = 0.0                                   # ACADOS default levenberg_marquardt
        self.qp_iter_max = 50                           # ACADOS default qp_solver_iter_max


class _OcpSolver:
    """The accessors the AL driver uses after compute_problem: get(i, 'x' | 'u')."""

    def __init__(self):
        self.x = self.u = None
        self.status = None

    def get(self, i, field):
        return np.copy(self.x[i] if field == "x" else self.u[i])

    def get_status(self):
        return self.status


class _AlOcp:
    """An AL OCP<chain>INIT class on the batched GPU solver (NQ: the chain): compute_problem(q0, v0) -> 1 / 0 / 2 and
    ocp_solver.get(i, 'x') of the step (vboc_al_solve_batch); compute_problem_batch for many states at once."""
    NQ = None

    def __init__(self, device=0, cost_scale=None):
        from .lib import Solver
        self.spec = AlSpec(self.NQ, cost_scale)
        s = self.spec
        self.N, self.nx, self.nu = s.N, s.nx, s.nu
        self.Tf, self.Cmax, self.thetamax, self.thetamin, self.dthetamax = (s.Tf, s.Cmax, s.thetamax, s.thetamin,
                                                                            s.dthetamax)
        self.device = device
        self.solver = Solver(self.NQ, self.N, device=device)
        self.solver.set_option("levenberg_marquardt", s.lm)
        self.solver.set_option("qp_solver_iter_max", s.qp_iter_max)
        self.solver.set_option("nlp_solver_tol_stat", 1e-6)    # ACADOS defaults (the class sets no tolerance)
        self.solver.set_option("qp_solver_tol_stat", 1e-8)
        self.ocp_solver = _OcpSolver()

    def compute_problem_batch(self, x0):
        """compute_problem for every row of x0 [B, 2nq] (numpy): dict(label, status, x [B, N+1, 2nq], u [B, N, nq],
        qp_iter) as numpy arrays."""
        import torch
        dev = torch.device("cuda", self.device)
        t = torch.as_tensor(np.ascontiguousarray(x0, dtype=np.float64), device=dev)
        out = self.solver.al_solve_device(self.spec, t)
        torch.cuda.synchronize(dev)
        return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}

    def labels(self, X):
        """(labels [B], trajectories [B, N+1, 2nq]) of compute_problem for every state of X: testing_batch's label_fn."""
        r = self.compute_problem_batch(X)
        return r["label"], r["x"]

    def _x0(self, q0, v0):
        n = self.NQ
        if n == 1:   # the pendulum's scalars (pendulum_class_al.py:147)
            return np.array([q0, v0], dtype=np.float64)
        return np.array([q0[j] for j in range(n)] + [v0[j] for j in range(n)], dtype=np.float64)   # :152

    def compute_problem(self, q0, v0):
        x0 = self._x0(q0, v0)
        r = self.compute_problem_batch(x0[None])
        self.ocp_solver.x, self.ocp_solver.u, self.ocp_solver.status = r["x"][0], r["u"][0], int(r["status"][0])
        return int(r["label"][0])

    def compute_problem_nnguess_batch(self, x0, model, mean, std):
        """compute_problem_nnguess (:171-201) for every row of x0 [B, 2nq]: the guess network's trajectory as every
        stage's x guess (nn_guess), then the same RTI step.  Returns the dict of compute_problem_batch."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        n = self.NQ
        xg = np.stack([nn_guess(self.N, s[:n], s[n:], model, mean, std) for s in x0]) if len(x0) else \
            np.zeros((0, self.N + 1, 2 * n))
        return self.compute_problem_guess_batch(x0, xg)

    def compute_problem_guess_batch(self, x0, xg):
        """The RTI step of compute_problem_nnguess from given stage guesses xg [B, N+1, 2nq] (stage 0 = x0)."""
        import torch
        dev = torch.device("cuda", self.device)
        T = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
        out = self.solver.al_solve_device(self.spec, T(x0), x_guess=T(xg))
        torch.cuda.synchronize(dev)
        return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}

    def labels_guess(self, X, xg):
        """(labels [B], trajectories [B, N+1, 2nq]) of the RTI step from the stage guesses xg for every state of X:
        the AL loop's testing_guess.  X and xg may be float64 device tensors (PoolScorer.guess's output): they go to
        the solver as they are, without visiting the host."""
        import torch
        dev = torch.device("cuda", self.device)
        T = lambda a: a.to(dev, torch.float64).contiguous() if torch.is_tensor(a) else \
            torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
        out = self.solver.al_solve_device(self.spec, T(X), x_guess=T(xg))
        torch.cuda.synchronize(dev)
        return out["label"].cpu().numpy(), out["x"].cpu().numpy()

    def compute_problem_nnguess(self, q0, v0, model, mean, std):
        x0 = self._x0(q0, v0)   # :175
        r = self.compute_problem_nnguess_batch(x0[None], model, mean, std)
        self.ocp_solver.x, self.ocp_solver.u, self.ocp_solver.status = r["x"][0], r["u"][0], int(r["status"][0])
        return int(r["label"][0])

    def labels_nnguess(self, model, mean, std):
        """testing_batch's label_fn for the driver's testing_guess (AL/triplependulum_al.py:44-62)."""
        def fn(X):
            r = self.compute_problem_nnguess_batch(X, model, mean, std)
            return r["label"], r["x"]
        return fn


class OCPtriplependulumINIT(_AlOcp):
    """AL's OCPtriplependulumINIT (AL/triplependulum_class_al.py:204-222; compute_problem :148-169,
    compute_problem_nnguess :171-201)."""
    NQ = 3


class OCPdoublependulumINIT(_AlOcp):
    """AL's OCPdoublependulumINIT (AL/doublependulum_class_al.py:402-420; compute_problem :206-227,
    compute_problem_nnguess :229-259) on the batched GPU solver.  compute_problem_withGUESS / _withGUESSPID are not
    built: no driver of the reference calls them."""
    NQ = 2

    def set_bounds(self, q_min, q_max):
        """:189-204 - the position box of both joints, on the path and at N.  As in the reference, only the OCP's
        constraints change: thetamin / thetamax (here and in the spec) keep the class's values, which is what the
        driver's out-of-bounds test reads (q_min, q_max = ocp.thetamin, ocp.thetamax, once, before any set_bounds)."""
        s = self.spec
        for j in range(2):
            s.xmin[j] = s.xmin_e[j] = q_min[j]
            s.xmax[j] = s.xmax_e[j] = q_max[j]


class OCPpendulumINIT(_AlOcp):
    """AL's OCPpendulumINIT (AL/pendulum_class_al.py:286-300; compute_problem(q0, v0) with scalar q0, v0 :143-164,
    compute_problem_nnguess :166-196) on the batched GPU solver."""
    NQ = 1

    def __init__(self, device=0, cost_scale=None):
        super().__init__(device, cost_scale)
        self.Fmax = self.spec.Fmax

    def set_bounds(self, q_min, q_max):
        """:127-141 - the position box on the path and at N; the reference also sets the instance's thetamin /
        thetamax (:128-129).  The spec's thetamin / thetamax, which out_of_bounds reads, keep the class's values, as
        for the double: the driver reads its q_min / q_max once, before any set_bounds."""
        s = self.spec
        self.thetamin, self.thetamax = q_min, q_max
        s.xmin[0] = s.xmin_e[0] = q_min
        s.xmax[0] = s.xmax_e[0] = q_max


def nn_guess(N, q0, v0, model, mean, std):
    """The stage guesses of compute_problem_nnguess (AL/triplependulum_class_al.py:180-192; the double's :238-250, the
    pendulum's :175-187): the guess network (NeuralNetCLS(2 nq, hidden, 2 nq N), FP32) evaluated on the normalised
    state exactly as the reference does it - one [1, 2 nq] float32 tensor, (x - mean) / std, model, * std + mean,
    reshaped to [N, 2 nq] - and x0 at stage 0.  q0, v0: nq values each (a pendulum's scalars as length-1 arrays).
    Evaluated on the model's device (the reference's is the CPU, where the FP32 arithmetic is the reference's own)."""
    import torch
    dev = next(model.parameters()).device
    s0 = [float(v) for v in np.ravel(q0)] + [float(v) for v in np.ravel(v0)]
    nx = len(s0)
    with torch.no_grad():
        inp = torch.Tensor([s0]).to(dev)
        inp = (inp - mean) / std
        out = model(inp)
        out = out * std + mean
        out = out.cpu().numpy()
    out = np.reshape(out, (N, nx))
    xg = np.empty((N + 1, nx))
    xg[0] = s0
    xg[1:] = out
    return xg


def out_of_bounds(spec, s0):
    """testing's pre-check (AL/triplependulum_al.py:27): a position outside [thetamin, thetamax] or a velocity outside
    [-dthetamax, dthetamax] on any joint."""
    n = spec.nq
    q0, v0 = s0[:n], s0[n:]
    q_min, q_max, v_min, v_max = spec.thetamin, spec.thetamax, -spec.dthetamax, spec.dthetamax
    return any(q0[j] < q_min or q0[j] > q_max or v0[j] < v_min or v0[j] > v_max for j in range(n))


def testing_batch(spec, S0, label_fn):
    """The AL driver's testing(s0) (AL/triplependulum_al.py:24-42) for every state of S0 [B, 6] at once:
    label_fn(x0 [b, 6]) -> (labels [b], x [b, N+1, 6]) solves the in-bounds states in one batch (compute_problem).
    Returns the list of testing's return values: ([q0, v0, 1, 0], None) for an out-of-bounds state or label 0,
    ([q0, v0, 0, 1], trajectory list of (N+1)*6) for label 1, and None for label 2 (testing falls off its if/elif)."""
    S0 = np.asarray(S0, dtype=np.float64)
    out = [None] * S0.shape[0]
    run = []
    for b, s0 in enumerate(S0):
        if out_of_bounds(spec, s0):
            out[b] = ([*map(float, s0), 1, 0], None)
        else:
            run.append(b)
    if run:
        labels, X = label_fn(S0[run])
        for j, b in enumerate(run):
            s0 = S0[b]
            if labels[j] == 1:
                out[b] = ([*map(float, s0), 0, 1], np.reshape(X[j], ((spec.N + 1) * spec.nx,)).tolist())
            elif labels[j] == 0:
                out[b] = ([*map(float, s0), 1, 0], None)
    return out


def unlabeled_states(spec, n, rng):
    """Samples in the driver's unlabeled box (AL/triplependulum_al.py:115-123): positions in [thetamin, thetamax],
    velocities in [-dthetamax, dthetamax] widened by 1/20 of the range on each side, uniform.  The double's driver
    scales a Halton sequence to the same box (AL/doublependulum_al.py:111-120); the pendulum's widens BOTH columns by
    1/100 of the velocity range (AL/pendulum_al.py:103-108).  The boxes are the drivers'; the draw here is uniform
    for every chain (the Halton sampler is scipy's and stays with the caller)."""
    v_min, v_max = -spec.dthetamax, spec.dthetamax
    nq = spec.nq
    if nq == 1:
        w = (v_max - v_min) / 100
        lo, hi = [spec.thetamin - w, v_min - w], [spec.thetamax + w, v_max + w]
    else:
        lo = [spec.thetamin] * nq + [v_min - (v_max - v_min) / 20] * nq
        hi = [spec.thetamax] * nq + [v_max + (v_max - v_min) / 20] * nq
    return rng.uniform(low=lo, high=hi, size=(n, 2 * nq))
