"""Safe MPC with the VBOC network as terminal constraint (VBOC/Safe MPC/), on the batched
solver.

The reference (`VBOC/Safe MPC/triplependulum_class_vboc.py`) wraps MODELtriplependulum (:8-78, nx 6, nu 3, the
VBOC triple's dynamics without the dt state) in an ACADOS OCP over tot_time / time_step intervals (:91-161):
  cost      LINEAR_LS, W = blockdiag(Q, R) at stages 0..N-1, W_e = Q at N (:108-134), Gauss-Newton Hessian:
            Q = diag(1e-4, 1e4, 1e-4, 1e-4, 1e-4, 1e-4), R = 1e-4 I, yref = [pi, thetamax - 0.05, pi, 0...]
  bounds    theta in [3pi/4, 5pi/4], |dtheta| <= 10 on the path and at N, |C| <= 10 (:136-151)
  options   qp_solver_iter_max 100, nlp_solver_max_iter 1000, MERIT_BACKTRACKING 0.3 / 1e-2,
            levenberg_marquardt 1e-2 (:153-161); the drivers pass "SQP_RTI"
            (hard_terminal_constraints/3dof_sym.py:96)
  OCP_solve(x0, x_sol_guess, u_sol_guess): x_0 fixed by constraints_set(0, lbx / ubx, x0), guesses at every
            stage (:163-181)
  HardTerm  the terminal row 0 <= NN(x_N) - max(|x_N[2:]|, 1e-3) <= 1e6 (:197-240; x[2:] includes theta_3 in the
            reference - kept)
The restatement: the free-time solver's model (dt a state, here pinned by x_0 and unbounded on the path - an
exact reformulation), its SQP / merit / Mehrotra IPM / Riccati recursion with the tracking cost's Gauss-Newton
Hessian and gradient and the terminal row handled like the Cartesian rows (oracle/vboc_oracle_ft.c,
vboc_amd/csrc/ft.h).  ACADOS' cost_scaling (stage costs times the time step in current releases, 1 in older
ones) is unpinned: `cost_scale` states the choice (default: the time step).  Under it the stage slack weights zl / Zl
of stages 0..N-1 are scaled too (stage N stays at 1), as ACADOS scales them; the receding driver, whose path slack
weights are large (10^(6(1 - ri/N)), 1e12), depends on that choice, so its closed-loop parity is unpinned as well.

The double pendulum (`VBOC/Safe MPC/<variant>/doublependulum_class_fixedveldir.py`, drivers `<variant>/2dof_sym.py`
for the five variants no_constraints, hard_terminal_constraints, soft_traj_constraints, receiding_hard_constraints and
parallel): the same OCP on four states - MpcSpec2, OCPdoublependulumINIT, SYMdoublependulumINIT and the 2dof closed
loops below.  Its OCP_solve takes the reference per call (q_ref), which the batched solver carries per problem
(vboc_mpc_batch_t.yref_b / yref_e_b).  The 2dof classes leave nlp_solver_type commented out: ACADOS' default,
SQP_RTI, is what they run ([EXT]: the default is ACADOS', not stated by the reference).
"""
import math

import numpy as np

from .systems import system


class MpcSpec:
    """The OCP data of OCPtriplependulum (Safe MPC/triplependulum_class_vboc.py:91-161) for a time step / horizon."""

    def __init__(self, time_step=4e-3, tot_time=0.148, cost_scale=None):
        s = system(3)
        self.nq = 3
        self.time_step, self.tot_time = float(time_step), float(tot_time)
        self.N = int(self.tot_time / self.time_step)                     # :105 dims.N = int(tot_time / time_step)
        self.thetamax, self.thetamin = math.pi / 4 + math.pi, -math.pi / 4 + math.pi   # :125-127
        self.dthetamax, self.Cmax = 10.0, 10.0
        self.Q = np.array([1e-4, 1e4, 1e-4, 1e-4, 1e-4, 1e-4])          # :111-112
        self.R = np.array([1e-4, 1e-4, 1e-4])
        self.W = np.concatenate([self.Q, self.R])
        self.W_e = self.Q.copy()
        self.yref = np.array([math.pi, self.thetamax - 0.05, math.pi, 0., 0., 0., 0., 0., 0.])   # :130-131
        self.yref_e = self.yref[:6].copy()
        self.xmax = np.array([self.thetamax] * 3 + [self.dthetamax] * 3)
        self.xmin = np.array([self.thetamin] * 3 + [-self.dthetamax] * 3)
        self.umax = np.full(3, self.Cmax)
        self.umin = -self.umax
        self.cost_scale = self.time_step if cost_scale is None else float(cost_scale)
        self.lm = 1e-2
        self.g, self.m, self.l = s.g, s.m, s.l


class MpcSpec2:
    """The OCP data of OCPdoublependulum (Safe MPC/<variant>/doublependulum_class_fixedveldir.py; the line numbers are
    no_constraints/'s, the five variants share them) for a horizon Tf: N = int(1000 Tf) intervals of Tf / N."""

    def __init__(self, Tf=0.01, cost_scale=None):
        s = system(2)
        self.nq = 2
        self.Tf = float(Tf)                                              # :120
        self.N = int(1000 * self.Tf)                                     # :121
        self.time_step = self.Tf / self.N
        self.tot_time = self.Tf
        self.thetamax, self.thetamin = math.pi / 4 + math.pi, -math.pi / 4 + math.pi   # :152-153
        self.dthetamax, self.Cmax = 10.0, 10.0                           # :151, :154
        self.Q = np.array([1e4, 1e4, 1e-4, 1e-4])                        # :131
        self.R = np.array([1e-4, 1e-4])                                  # :132
        self.W = np.concatenate([self.Q, self.R])
        self.W_e = self.Q.copy()
        self.yref = np.array([math.pi, math.pi, 0., 0., 0., 0.])         # :147 (OCP_solve replaces it with q_ref)
        self.yref_e = self.yref[:4].copy()                               # :148
        self.xmax = np.array([self.thetamax] * 2 + [self.dthetamax] * 2)
        self.xmin = np.array([self.thetamin] * 2 + [-self.dthetamax] * 2)
        self.umax = np.full(2, self.Cmax)
        self.umin = -self.umax
        self.cost_scale = self.time_step if cost_scale is None else float(cost_scale)
        self.lm = 1.0                                                    # :185 levenberg_marquardt
        self.tol = 1e-2                                                  # :179 the four NLP tolerances
        self.qp_iter_max, self.max_iter = 100, 1000                      # :180-181
        self.alpha_reduction, self.alpha_min = 0.3, 1e-2                 # :183-184
        self.g, self.m, self.l = s.g, s.m, s.l

    def references(self, q_ref):
        """OCP_solve's cost_set(i, 'y_ref', [q_ref, 0, 0, 0, 0]) / (N, 'y_ref', [q_ref, 0, 0]) (:205, :208) for the
        rows of q_ref [B, 2]: (yref [B, 6], yref_e [B, 4])."""
        q = np.atleast_2d(np.asarray(q_ref, dtype=np.float64))
        yr, yre = np.zeros((q.shape[0], 6)), np.zeros((q.shape[0], 4))
        yr[:, :2] = yre[:, :2] = q
        return yr, yre

    def gravity_torque(self, x):
        """The drivers' control guess at a state: gravity compensation (2dof_sym.py:30), in their order of operations
        (math.sin, left to right)."""
        g, (m1, m2), (l1, l2) = self.g, self.m, self.l
        return np.array([g * l1 * (m1 + m2) * math.sin(x[0]), g * l2 * m2 * math.sin(x[1])])


def nn_params(model):
    """The six NeuralNetDIR parameters (list(model.parameters()), the reference's nn_params) as float64 arrays:
    CasADi's SX(param.tolist()) takes the float32 values exactly."""
    return [np.ascontiguousarray(p.detach().cpu().numpy().astype(np.float64)) for p in model.parameters()]


def nn_row(params, mean, std, x, safety_margin=None):
    """h(x) = nn_decisionfunction(params, mean, std, x) (:208-230) for one state x [2 nq] (numpy); with safety_margin
    the SoftTraj class's nn_decisionfunction_conservative (:284-304): out * (100 - safety_margin) / 100 - vn.  The
    receding driver evaluates it on the previous solution's states (receiding_hard_constraints/3dof_sym.py:32-35).
    x[2:] is the reference's for every chain: theta_3 and the velocities for the triple, the velocity pair for the
    double (doublependulum_class_fixedveldir.py nn_decisionfunction)."""
    x = np.asarray(x, dtype=np.float64)
    nq = x.shape[0] // 2
    vn = max(float(np.linalg.norm(x[2:])), 1e-3)
    z = np.concatenate([(x[:nq] - mean) / std, x[nq:] / vn])
    W0, b0, W1, b1, W2, b2 = params
    a = np.maximum(W0 @ z + b0, 0.0)
    a = np.maximum(W1 @ a + b1, 0.0)
    out = float((W2 @ a + b2)[0])
    if safety_margin is not None:
        out = out * (100 - safety_margin) / 100
    return out - vn


# ------------------------------------------------------------------------------------------------
# drop-in classes (Safe MPC/triplependulum_class_vboc.py:81-240) on the GPU solver, batch of one
# ------------------------------------------------------------------------------------------------
class _Dims:
    def __init__(self, N, nx, nu):
        self.N, self.nx, self.nu = N, nx, nu


class _Ocp:
    def __init__(self, spec):
        self.dims = _Dims(spec.N, 2 * spec.nq, spec.nq)


class _OcpSolver:
    """The ocp_solver accessors the Safe-MPC drivers use: get(i, 'x' | 'u') of the last OCP_solve."""

    def __init__(self):
        self.x = self.u = None
        self.cost = None

    def get(self, i, field):
        return np.copy(self.x[i] if field == "x" else self.u[i])

    def get_cost(self):
        return self.cost


class OCPtriplependulum:
    """OCPtriplependulum (:81-181) on the batched GPU solver (vboc_mpc_solve_batch): OCP_solve(x0, x_sol_guess,
    u_sol_guess) -> status, results through ocp_solver.get.  nn_params None: OCPtriplependulumSTD (no terminal row)."""

    def __init__(self, nlp_solver_type, time_step, tot_time, nn_params=None, mean=0.0, std=1.0, regenerate=False,
                 cost_scale=None, device=0):
        import torch
        from .lib import Solver
        self.spec = MpcSpec(time_step, tot_time, cost_scale)
        self.N = self.spec.N
        self.ocp = _Ocp(self.spec)
        self.rti = nlp_solver_type == "SQP_RTI"
        self.thetamax, self.thetamin, self.dthetamax, self.Cmax = (self.spec.thetamax, self.spec.thetamin,
                                                                   self.spec.dthetamax, self.spec.Cmax)
        self.Xmax_limits, self.Xmin_limits = self.spec.xmax, self.spec.xmin
        self.dev = torch.device("cuda", device)
        self.solver = Solver(3, max(self.N, 2), device=device)
        self.solver.set_option("levenberg_marquardt", self.spec.lm)
        self.solver.set_option("nlp_solver_tol_stat", 1e-6)       # ACADOS defaults (the class sets no tolerance)
        self.solver.set_option("qp_solver_tol_stat", 1e-8)
        self.params = None
        if nn_params is not None:
            self.params = [torch.as_tensor(np.asarray(p, dtype=np.float64), device=self.dev) for p in nn_params]
        self.mean, self.std = float(mean), float(std)
        self.ocp_solver = _OcpSolver()

    def solve_batch(self, x0, x_guess, u_guess):
        """Batched OCP_solve: numpy [B, 6], [B, N+1, 6], [B, N, 3] -> dict of numpy results."""
        import torch
        T = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=self.dev)
        out = self.solver.mpc_solve_device(self.spec, T(x0), T(x_guess), T(u_guess), self.params, self.mean,
                                           self.std, rti=self.rti)
        torch.cuda.synchronize(self.dev)
        return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}

    def OCP_solve(self, x0, x_sol_guess, u_sol_guess):
        r = self.solve_batch(np.asarray(x0)[None], np.asarray(x_sol_guess)[None], np.asarray(u_sol_guess)[None])
        self.ocp_solver.x, self.ocp_solver.u, self.ocp_solver.cost = r["x"][0], r["u"][0], float(r["cost"][0])
        return int(r["status"][0])


class OCPtriplependulumHardTerm(OCPtriplependulum):
    """The hard terminal constraint class (:197-240): NN(x_N) - max(|x_N[2:]|, 1e-3) in [0, 1e6]."""

    def __init__(self, nlp_solver_type, time_step, tot_time, nn_params, mean, std, regenerate=False, **kw):
        super().__init__(nlp_solver_type, time_step, tot_time, nn_params=[np.asarray(p.detach().cpu().numpy()
                         if hasattr(p, "detach") else p, dtype=np.float64) for p in nn_params],
                         mean=float(mean), std=float(std), regenerate=regenerate, **kw)


class _SoftOcpSolver(_OcpSolver):
    """The SoftTraj drivers' accessors: get(i, 'x' | 'u') and cost_set(i, 'Zl' | 'zl' | 'W', value) - the per-stage
    slack weights (soft_traj_constraints/3dof_sym.py:102-105, receiding_hard_constraints/3dof_sym.py:41-46) and stage
    weights (:36-40), kept until changed, as ACADOS keeps them in the solver."""

    def __init__(self, ocp):
        super().__init__()
        self.ocp = ocp

    def cost_set(self, i, field, value):
        o, N = self.ocp, self.ocp.N
        if not 0 <= i <= N:
            raise ValueError(f"stage {i} outside 0..{N}")
        v = np.asarray(value, dtype=np.float64)
        if field in ("Zl", "zl"):
            getattr(o, field)[i] = float(v.reshape(-1)[0])
        elif field == "W":
            if np.abs(v - np.diag(np.diag(v))).max() > 0.0:
                raise NotImplementedError("cost_set(W): diagonal weights only (the drivers' block_diag(Q, R))")
            if i < N:
                o.W[i] = np.diag(v)
            else:
                o.We[:] = np.diag(v)
        else:
            raise NotImplementedError(f"cost_set field {field!r}")


class OCPtriplependulumSoftTraj(OCPtriplependulum):
    """The soft-constraint class (:242-304): the row nn_decisionfunction_conservative = NN(x) (100 - safety_margin) /
    100 - max(|x[2:]|, 1e-3) on every stage 0..N (con_h_expr and con_h_expr_e, lh = 0, uh = 1e6), soft on its lower
    side (idxsh / idxsh_e) with zl = Zl = zu = Zu = 0 until the driver sets them (ocp_solver.cost_set).  GPU:
    vboc_mpc_soft_solve_batch (ft.h)."""

    def __init__(self, nlp_solver_type, time_step, tot_time, nn_params, mean, std, safety_margin, regenerate=False,
                 **kw):
        super().__init__(nlp_solver_type, time_step, tot_time, nn_params=[np.asarray(p.detach().cpu().numpy()
                         if hasattr(p, "detach") else p, dtype=np.float64) for p in nn_params],
                         mean=float(mean), std=float(std), regenerate=regenerate, **kw)
        self.safety_margin = float(safety_margin)
        N = self.N
        self.Zl, self.zl = np.zeros(N + 1), np.zeros(N + 1)     # ocp.cost.Zl / zl / Zl_e / zl_e = 0 (:265-282)
        self.W = np.tile(self.spec.W, (N, 1))
        self.We = self.spec.W_e.copy()
        self.ocp_solver = _SoftOcpSolver(self)

    def nn_decisionfunction_conservative(self, params, mean, std, safety_margin, x):
        """The row at one state (:284-304), numerically (the receding driver's use, :32-35)."""
        P = [np.asarray(p.detach().cpu().numpy() if hasattr(p, "detach") else p, dtype=np.float64) for p in params]
        return nn_row(P, float(mean), float(std), x, safety_margin=safety_margin)

    def weights(self, B):
        """The solver's current weights as per-problem arrays (Zl, zl [B, N+1], W [B, 9], We [B, 6])."""
        if np.abs(self.W - self.W[0]).max() > 0.0:
            raise NotImplementedError("different stage weights W on different stages")
        return dict(Zl=np.tile(self.Zl, (B, 1)), zl=np.tile(self.zl, (B, 1)), W=np.tile(self.W[0], (B, 1)),
                    We=np.tile(self.We, (B, 1)))

    def solve_batch(self, x0, x_guess, u_guess, weights=None):
        """Batched OCP_solve: numpy [B, 6], [B, N+1, 6], [B, N, 3]; weights: per-problem arrays (Zl, zl, W, We;
        default: the solver's, cost_set)."""
        import torch
        B = np.asarray(x0).shape[0]
        w = self.weights(B)
        if weights is not None:
            w.update({k: np.asarray(v, dtype=np.float64) for k, v in weights.items() if v is not None})
        T = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=self.dev)
        soft = dict(margin=self.safety_margin, **{k: T(v) for k, v in w.items()})
        out = self.solver.mpc_solve_device(self.spec, T(x0), T(x_guess), T(u_guess), self.params, self.mean,
                                           self.std, rti=self.rti, soft=soft)
        torch.cuda.synchronize(self.dev)
        return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


class _Integrator:
    def __init__(self, T, nq=3):
        self.T, self.nq, self.x, self.u, self.out = T, nq, None, None, None

    def set(self, field, v):
        if field == "T":
            self.T = float(v)
        else:
            setattr(self, field, np.asarray(v, dtype=np.float64))

    def solve(self):
        from .lib import rk4_host
        self.out = rk4_host(self.nq, self.T, self.x[None], self.u[None])[0]
        return 0

    def get(self, field):
        return np.copy(self.out)


class OCPdoublependulumINIT:
    """OCPdoublependulumINIT of VBOC/Safe MPC/<variant>/doublependulum_class_fixedveldir.py on the batched GPU solver
    (k_ftr<2>), in the reference's three shapes:
      OCPdoublependulumINIT(regenerate)                                          no_constraints/: no row;
      OCPdoublependulumINIT(regenerate, nn_params, mean, std, safety_margin)     hard_terminal_constraints/: the row
            NN(x_N) - max(|x_N[2:]|, 1e-3) in [0, 1e6] at N (safety_margin is taken and unused, as there);
      OCPdoublependulumINIT(regenerate, nn_params, mean, std, safety_margin, soft=True)   soft_traj_constraints/,
            receiding_hard_constraints/, parallel/: the margin-scaled row on every stage, soft lower sides with
            zl = Zl = 0 until cost_set ([EXT] the keyword: the reference picks the shape by folder).
    OCP_solve(x0, q_ref, x_sol_guess, u_sol_guess) -> status; ocp_solver.get(i, 'x' | 'u'), ocp_solver.cost_set(i,
    'Zl' | 'zl' | 'W', value).  nlp_solver_type: the classes leave it commented out - ACADOS' default SQP_RTI."""

    def __init__(self, regenerate=False, nn_params=None, mean=0.0, std=1.0, safety_margin=None, soft=False,
                 nlp_solver_type="SQP_RTI", Tf=0.01, cost_scale=None, device=0):
        import torch
        from .lib import Solver
        self.spec = sp = MpcSpec2(Tf, cost_scale)
        self.N, self.nx, self.nu = sp.N, 4, 2
        self.ocp = _Ocp(sp)
        self.rti = nlp_solver_type == "SQP_RTI"
        self.thetamax, self.thetamin, self.dthetamax, self.Cmax = sp.thetamax, sp.thetamin, sp.dthetamax, sp.Cmax
        self.g, (self.m1, self.m2), (self.l1, self.l2) = sp.g, sp.m, sp.l
        self.dev = torch.device("cuda", device)
        self.solver = Solver(2, max(self.N, 2), device=device)
        self.solver.set_option("levenberg_marquardt", sp.lm)
        for t_ in ("stat", "eq", "ineq", "comp"):
            self.solver.set_option(f"nlp_solver_tol_{t_}", sp.tol)
        self.solver.set_option("qp_solver_iter_max", sp.qp_iter_max)
        self.solver.set_option("nlp_solver_max_iter", sp.max_iter)
        self.solver.set_option("qp_solver_tol_stat", 1e-8)        # ACADOS default (the class sets no QP tolerance)
        self.params = None
        if nn_params is not None:
            self.params = [torch.as_tensor(np.asarray(p.detach().cpu().numpy() if hasattr(p, "detach") else p,
                                                      dtype=np.float64), device=self.dev) for p in nn_params]
        elif soft:
            raise ValueError("the soft rows need the network (nn_params)")
        self.mean, self.std = float(mean), float(std)
        self.soft = bool(soft)
        self.safety_margin = None if safety_margin is None else float(safety_margin)
        if self.soft:
            if self.safety_margin is None:
                raise ValueError("the soft rows need safety_margin")
            self.Zl, self.zl = np.zeros(self.N + 1), np.zeros(self.N + 1)
            self.W = np.tile(sp.W, (self.N, 1))
            self.We = sp.W_e.copy()
            self.ocp_solver = _SoftOcpSolver(self)
        else:
            self.ocp_solver = _OcpSolver()

    def nn_decisionfunction(self, params, mean, std, safety_margin, x):
        """The row at one state, numerically (the receding and parallel drivers' use): the soft shape's is
        margin-scaled, the hard-terminal shape's is not (it takes safety_margin and ignores it)."""
        P = [np.asarray(p.detach().cpu().numpy() if hasattr(p, "detach") else p, dtype=np.float64) for p in params]
        return nn_row(P, float(mean), float(std), x, safety_margin=safety_margin if self.soft else None)

    def weights(self, B):
        """The soft shape's current weights as per-problem arrays (Zl, zl [B, N+1], W [B, 6], We [B, 4])."""
        if np.abs(self.W - self.W[0]).max() > 0.0:
            raise NotImplementedError("different stage weights W on different stages")
        return dict(Zl=np.tile(self.Zl, (B, 1)), zl=np.tile(self.zl, (B, 1)), W=np.tile(self.W[0], (B, 1)),
                    We=np.tile(self.We, (B, 1)))

    def solve_batch(self, x0, x_guess, u_guess, weights=None, q_ref=None):
        """Batched OCP_solve: numpy [B, 4], [B, N+1, 4], [B, N, 2]; q_ref [B, 2] (or [2]: the same for every problem;
        None: the class's yref): each problem's reference.  weights (soft shape): per-problem arrays (Zl, zl, W, We;
        default: the solver's, cost_set)."""
        import torch
        B = np.asarray(x0).shape[0]
        T = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=self.dev)
        yr = yre = None
        if q_ref is not None:
            yr, yre = self.spec.references(np.broadcast_to(np.asarray(q_ref, dtype=np.float64), (B, 2)))
            yr, yre = T(yr), T(yre)
        soft = None
        if self.soft:
            w = self.weights(B)
            if weights is not None:
                w.update({k: np.asarray(v, dtype=np.float64) for k, v in weights.items() if v is not None})
            soft = dict(margin=self.safety_margin, **{k: T(v) for k, v in w.items()})
        out = self.solver.mpc_solve_device(self.spec, T(x0), T(x_guess), T(u_guess), self.params, self.mean, self.std,
                                           rti=self.rti, soft=soft, yref=yr, yref_e=yre)
        torch.cuda.synchronize(self.dev)
        return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}

    def OCP_solve(self, x0, q_ref, x_sol_guess, u_sol_guess):
        r = self.solve_batch(np.asarray(x0)[None], np.asarray(x_sol_guess)[None], np.asarray(u_sol_guess)[None],
                             q_ref=np.asarray(q_ref)[None])
        self.ocp_solver.x, self.ocp_solver.u, self.ocp_solver.cost = r["x"][0], r["u"][0], float(r["cost"][0])
        return int(r["status"][0])


class SYMdoublependulumINIT:
    """SYMdoublependulumINIT (doublependulum_class_fixedveldir.py:216-226): one ERK4 step of T = 1e-3."""

    def __init__(self, regenerate=False):
        self.acados_integrator = _Integrator(1e-3, 2)


class SYMtriplependulum:
    """SYMtriplependulum (:70-78): one ERK4 step of T = time_step (vboc_rk4_batch)."""

    def __init__(self, time_step, tot_time, regenerate=False):
        self.acados_integrator = _Integrator(time_step)


# ------------------------------------------------------------------------------------------------
# the closed-loop driver (hard_terminal_constraints/3dof_sym.py:15-72) for a batch of initial states
# ------------------------------------------------------------------------------------------------
def simulate_batch(solve, rk4, spec, x0s, x_guess, u_guess, tot_steps=100, weights=None, log=None, tail_u=None,
                   failed_start=-1, stop_at_first=False):
    """The reference's simulate(p) for every initial state at once: each MPC step solves the OCPs of the problems
    still running in one batched call (solve(x0 [b, 6], xg [b, N+1, 6], ug [b, N, 3]) -> dict(status, x, u)),
    applies the reference's guess shifting and failure bookkeeping per problem (failed_iter, :37-62), and steps the
    plant with one RK4 of time_step (rk4(x [b, 6], u [b, 3]) -> x1).  Returns (res_steps [B] - the step at which each
    problem stopped, as simulate returns f -, simX [B, tot_steps + 1, 6], solves).
    weights (the receding driver): weights(f, failed [b], last_x [b, N+1, 6]) -> per-problem solver weights for the
    step, passed as solve(x0, xg, ug, weights); last_x is each problem's previous solve's result (ocp_solver.get).
    log (dict, optional) receives 'u' [B, tot_steps, 3]: the control applied to the plant at each step (NaN after the
    stop).
    The widths are the states' (6 / 3 for the triple, 4 / 2 for the double).  What the 2dof simulate functions do
    differently (VBOC/Safe MPC/<variant>/2dof_sym.py; simulate2_batch sets these):
      tail_u(x) - the last control guess is recomputed at x_sol_guess[N-1] (gravity compensation, :54, :68) instead of
                  copied from stage N-2 on success and left as shifted on failure;
      failed_start - failed_iter starts at -1 (no_constraints/, hard_terminal_constraints/, soft_traj_constraints/) or
                  0 (receiding_hard_constraints/, parallel/);
      stop_at_first - with failed_iter started at 0 the drivers stop a problem whose FIRST solve fails by `f == 0`
                  where the others test `failed_iter < 0` (receiding_hard_constraints/2dof_sym.py:67)."""
    x0s = np.asarray(x0s, dtype=np.float64)
    B, N = x0s.shape[0], spec.N
    xg = np.array(x_guess, dtype=np.float64, copy=True)
    ug = np.array(u_guess, dtype=np.float64, copy=True)
    nx, nu = x0s.shape[1], np.asarray(u_guess).shape[2]
    simX = np.zeros((B, tot_steps + 1, nx))
    simX[:, 0] = x0s
    failed = np.full(B, failed_start)
    res = np.full(B, tot_steps - 1)
    live = np.ones(B, dtype=bool)
    last_x = np.array(xg, copy=True)
    appliedU = np.full((B, tot_steps, nu), np.nan)
    solves = 0
    for f in range(tot_steps):
        idx = np.flatnonzero(live)
        if idx.size == 0:
            break
        if weights is None:
            r = solve(simX[idx, f], xg[idx], ug[idx])
        else:
            r = solve(simX[idx, f], xg[idx], ug[idx], weights(f, failed[idx], last_x[idx]))
        last_x[idx] = r["x"]
        solves += idx.size
        simU = np.zeros((idx.size, nu))
        keep = np.ones(idx.size, dtype=bool)
        for j, b in enumerate(idx):
            if r["status"][j] != 0:
                if failed[b] >= N - 1 or (f == 0 if stop_at_first else failed[b] < 0):
                    res[b] = f
                    live[b] = False
                    keep[j] = False
                    continue
                failed[b] += 1
                simU[j] = ug[b, 0]
                xg[b, :N - 1] = xg[b, 1:N].copy()
                ug[b, :N - 1] = ug[b, 1:N].copy()
                xg[b, N - 1] = xg[b, N]
                if tail_u is not None:
                    ug[b, N - 1] = tail_u(xg[b, N - 1])
            else:
                failed[b] = 0
                simU[j] = r["u"][j, 0]
                xg[b, :N - 1] = r["x"][j, 1:N]
                ug[b, :N - 1] = r["u"][j, 1:N]
                xg[b, N - 1] = r["x"][j, N]
                xg[b, N] = xg[b, N - 1]
                ug[b, N - 1] = ug[b, N - 2] if tail_u is None else tail_u(xg[b, N - 1])
        step = idx[keep]
        if step.size:
            simX[step, f + 1] = rk4(simX[step, f], simU[keep])
            appliedU[step, f] = simU[keep]
    if log is not None:
        log["u"] = appliedU
    return res, simX, solves


# ------------------------------------------------------------------------------------------------
# the soft-constraint drivers (VBOC/Safe MPC/soft_traj_constraints/3dof_sym.py, receiding_hard_constraints/3dof_sym.py)
# ------------------------------------------------------------------------------------------------
def soft_traj_weights(N):
    """soft_traj_constraints/3dof_sym.py:102-105: Zl = 0 on stages 1..N-1, 1e6 at N (stage 0 keeps the class's 0)."""
    Zl = np.zeros(N + 1)
    Zl[N] = 1e6
    return Zl


def receding_weights(params, mean, std, safety_margin, N, nq=3):
    """receiding_hard_constraints/3dof_sym.py:26-46 for the problems of one MPC step: the receding index from the
    previous solution (the last stage i in 1..N whose state satisfies the row, when the previous solve succeeded),
    receiding_iter = N - failed_iter - receiding, Q = diag(1e-2 + 10^(2 receiding_iter / N), 1e-4, ...), R = 1e-4 I,
    Zl = 1e12 at stage receiding_iter and 10^(6 (1 - receiding_iter / N)) elsewhere.  Returns weights(f, failed,
    last_x) for simulate_batch.  nq = 2 (receiding_hard_constraints/2dof_sym.py:39-57): the same with the position
    weight on BOTH joints, Q = diag(q, q, 1e-4, 1e-4)."""
    def weights(f, failed, last_x):
        b = failed.shape[0]
        Zl, W, We = np.empty((b, N + 1)), np.empty((b, 3 * nq)), np.empty((b, 2 * nq))
        for j in range(b):
            receiding = 0
            fi = int(failed[j])
            if fi == 0 and f > 0:
                for i in range(1, N + 1):
                    if nn_row(params, mean, std, last_x[j, i], safety_margin=safety_margin) >= 0.:
                        receiding = N - i + 1
            ri = N - fi - receiding
            Q = np.full(2 * nq, 1e-4)
            Q[:1 if nq == 3 else 2] = 1e-2 + pow(10, ri / N * 2)
            W[j] = np.r_[Q, [1e-4] * nq]
            We[j] = Q
            Zl[j] = pow(10, (1 - ri / N) * 6)
            if 0 <= ri <= N:
                Zl[j, ri] = 1e12
        return dict(Zl=Zl, W=W, We=We)
    return weights


def halton_states(spec, test_num=100):
    """The drivers' initial states (:98-103): a Halton sequence (scipy.stats.qmc, unscrambled) of the positions
    scaled to [Xmin, Xmax], zero velocities."""
    from scipy.stats import qmc
    sample = qmc.Halton(d=3, scramble=False).random(n=test_num)
    data = qmc.scale(sample, spec.xmin[:3], spec.xmax[:3])
    x0 = np.zeros((test_num, 6))
    x0[:, :3] = data
    return x0


def compare_steps(res_steps_traj, res_steps):
    """The drivers' comparison with the unconstrained MPC (:158-172): better / equal / worse counts."""
    d = np.asarray(res_steps_traj) - np.asarray(res_steps)
    return int((d > 0).sum()), int((d == 0).sum()), int((d < 0).sum())


# ------------------------------------------------------------------------------------------------
# the double pendulum's closed loops (VBOC/Safe MPC/<variant>/2dof_sym.py)
# ------------------------------------------------------------------------------------------------
def halton_states2(spec, test_num=100):
    """The 2dof drivers' initial states (2dof_sym.py:17, :87-94): Halton positions (d = 2, unscrambled) scaled to the
    position box, both velocities 1e-10."""
    from scipy.stats import qmc
    sample = qmc.Halton(d=2, scramble=False).random(n=test_num)
    x0 = np.full((test_num, 4), 1e-10)
    x0[:, :2] = qmc.scale(sample, [spec.thetamin] * 2, [spec.thetamax] * 2)
    return x0


def driver_q_ref(spec):
    """q_ref of the 2dof drivers (2dof_sym.py:99): the box's middle on joint 1, thetamax - 0.05 on joint 2."""
    return np.array([(spec.thetamax + spec.thetamin) / 2, spec.thetamax - 0.05])


def initial_guess2(spec, x0s):
    """The 2dof drivers' guesses (:28-30): the initial state at every stage, gravity compensation there as every
    control."""
    x0s = np.asarray(x0s, dtype=np.float64)
    xg = np.repeat(x0s[:, None, :], spec.N + 1, 1)
    ug = np.repeat(np.stack([spec.gravity_torque(x) for x in x0s])[:, None, :], spec.N, 1)
    return xg, ug


def soft_traj_weights2(N):
    """soft_traj_constraints/2dof_sym.py:109-111: Zl = 1e6 on stages 1..N (stage 0 keeps the class's 0)."""
    Zl = np.full(N + 1, 1e6)
    Zl[0] = 0.0
    return Zl


def simulate2_batch(kind, solve, rk4, spec, x0s, tot_steps=100, row=None, log=None):
    """simulate(p) of VBOC/Safe MPC/<kind>/2dof_sym.py for every initial state at once; kind: 'no_constraints',
    'hard_terminal_constraints', 'soft_traj_constraints' (the caller's solve carries soft_traj_weights2),
    'receiding_hard_constraints' or 'parallel'.  solve(x0 [b, 4], xg, ug[, weights]) -> dict(status, x, u) solves with
    the drivers' q_ref; row(x [4]) -> the margin-scaled row at a state (the receding and parallel drivers).  Returns
    simulate_batch's (res_steps, simX, solves)."""
    xg, ug = initial_guess2(spec, x0s)
    if kind == "parallel":
        return simulate_parallel_batch(solve, rk4, spec, x0s, xg, ug, row, tot_steps=tot_steps, log=log)
    rec = kind == "receiding_hard_constraints"
    weights = None
    if rec:
        def weights(f, failed, last_x):
            b = failed.shape[0]
            Zl, W, We = np.empty((b, spec.N + 1)), np.empty((b, 6)), np.empty((b, 4))
            for j in range(b):
                Zl[j], W[j], We[j], _ = _receding_step2(spec.N, int(failed[j]), f, last_x[j], row)
            return dict(Zl=Zl, W=W, We=We)
    return simulate_batch(solve, rk4, spec, x0s, xg, ug, tot_steps=tot_steps, weights=weights, log=log,
                          tail_u=spec.gravity_torque, failed_start=0 if rec else -1, stop_at_first=rec)


def _receding_step2(N, failed_iter, f, last_x, row):
    """receiding_hard_constraints/2dof_sym.py:35-57 for one problem: (Zl [N+1], W [6], We [4], receiding_iter)."""
    receiding = 0
    if failed_iter == 0 and f > 0:
        for i in range(1, N + 1):
            if row(last_x[i]) >= 0.:
                receiding = N - i + 1
    ri = N - failed_iter - receiding
    q = 1e-2 + pow(10, ri / N * 2)
    Q = np.array([q, q, 1e-4, 1e-4])
    Zl = np.full(N + 1, pow(10, (1 - ri / N) * 6))
    if 0 <= ri <= N:
        Zl[ri] = 1e12
    return Zl, np.r_[Q, [1e-4, 1e-4]], Q, ri


def parallel_candidates(N, receiding_iter):
    """parallel/2dof_sym.py:44-51: the placements p of the one stiff slack weight, in the driver's order
    reversed(range(receiding_iter, N + 1)), as rows Zl [n, N+1] (1e9 at p, 0 elsewhere)."""
    ps = list(reversed(range(receiding_iter, N + 1)))
    Zl = np.zeros((len(ps), N + 1))
    for c, p_ in enumerate(ps):
        if p_ >= 0:   # receiding_iter < 0 (receiding = N + 1 after a row satisfied at stage 0): no stage matches `i == p`
            Zl[c, p_] = 1e9
    return ps, Zl


def simulate_parallel_batch(solve, rk4, spec, x0s, x_guess, u_guess, row, tot_steps=100, log=None, sequential=False):
    """parallel/2dof_sym.py simulate(p) for every initial state at once.  At each MPC step the reference retries the
    OCP over the placements of one stiff slack weight (parallel_candidates) and takes the first that returns status 0;
    the candidates of one problem share x0, guesses and stage weights and differ only in Zl, so here the candidates of
    ALL live problems are solved in ONE batched call (per-problem Zl, W, We) and each problem takes its first status-0
    candidate in the reference's order - the sequential retry's result by construction (sequential=True runs the
    retry candidate by candidate, for the tests).  receiding persists across steps (:25, :57-60), failed_iter starts at
    0 and a problem stops when every candidate fails at f == 0 or after N - 1 consecutive failures (:81)."""
    x0s = np.asarray(x0s, dtype=np.float64)
    B, N = x0s.shape[0], spec.N
    xg = np.array(x_guess, dtype=np.float64, copy=True)
    ug = np.array(u_guess, dtype=np.float64, copy=True)
    simX = np.zeros((B, tot_steps + 1, 4))
    simX[:, 0] = x0s
    failed, receiding = np.zeros(B, dtype=int), np.zeros(B, dtype=int)
    res = np.full(B, tot_steps - 1)
    live = np.ones(B, dtype=bool)
    appliedU = np.full((B, tot_steps, 2), np.nan)
    solves = 0
    for f in range(tot_steps):
        idx = np.flatnonzero(live)
        if idx.size == 0:
            break
        owner, Zl, W, We, ris = [], [], [], [], {}
        for b in idx:
            ri = N - failed[b] - receiding[b]
            ris[b] = ri
            q = 1e-2 + pow(10, ri / N * 2)
            Q = np.array([q, q, 1e-4, 1e-4])
            _, Z = parallel_candidates(N, ri)
            owner += [b] * Z.shape[0]
            Zl.append(Z)
            W += [np.r_[Q, [1e-4, 1e-4]]] * Z.shape[0]
            We += [Q] * Z.shape[0]
        owner, Zl, W, We = np.array(owner), np.concatenate(Zl), np.array(W), np.array(We)
        if sequential:
            status = np.full(owner.size, -1)
            X, U = np.zeros((owner.size, N + 1, 4)), np.zeros((owner.size, N, 2))
            done = set()
            for c, b in enumerate(owner):
                if b in done:
                    continue
                r = solve(simX[b:b + 1, f], xg[b:b + 1], ug[b:b + 1], dict(Zl=Zl[c:c + 1], W=W[c:c + 1], We=We[c:c + 1]))
                solves += 1
                status[c], X[c], U[c] = r["status"][0], r["x"][0], r["u"][0]
                if status[c] == 0:
                    done.add(b)
        else:
            r = solve(simX[owner, f], xg[owner], ug[owner], dict(Zl=Zl, W=W, We=We))
            solves += owner.size
            status, X, U = r["status"], r["x"], r["u"]
        step, simU = [], []
        for b in idx:
            ok = np.flatnonzero((owner == b) & (status == 0))
            if ok.size == 0:
                if failed[b] >= N - 1 or f == 0:
                    res[b] = f
                    live[b] = False
                    continue
                failed[b] += 1
                u0 = ug[b, 0].copy()
                xg[b, :N - 1] = xg[b, 1:N].copy()
                ug[b, :N - 1] = ug[b, 1:N].copy()
                xg[b, N - 1] = xg[b, N]
            else:
                c = ok[0]
                for l in reversed(range(max(ris[b], 0), N + 1)):
                    if row(X[c, l]) >= 0.:
                        receiding[b] = N - l + 1
                        break
                failed[b] = 0
                u0 = U[c, 0].copy()
                xg[b, :N - 1] = X[c, 1:N]
                ug[b, :N - 1] = U[c, 1:N]
                xg[b, N - 1] = X[c, N]
                xg[b, N] = xg[b, N - 1]
            ug[b, N - 1] = spec.gravity_torque(xg[b, N - 1])
            step.append(b)
            simU.append(u0)
        if step:
            simX[step, f + 1] = rk4(simX[step, f], np.array(simU))
            appliedU[step, f] = np.array(simU)
    if log is not None:
        log["u"] = appliedU
    return res, simX, solves
