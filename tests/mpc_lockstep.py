"""Per-step lockstep of a Safe-MPC closed loop on two solvers (test helper; the rules are tests/test_safempc.py's, which
keeps its own copy for the triple): the loop runs on the first solver, and every MPC step's OCP is also solved by the
second from the SAME inputs (state, shifted guesses, weights).  Each step pair is classified:
  same    - equal status; for status 0 the applied u_0 and the predicted states agree to STEP_TOL;
  cap     - a QP stopped at qp_solver_iter_max (100) - an unconverged interior-point iterate, which rounding moves
            freely - while the other solver's QP also needed >= 50 iterations (a QP hard for both);
  status  - the solvers returned different statuses for the same request;
  value   - anything else: a defect.
STEP_TOL: an RTI QP converged to qp_tol_stat 1e-8 on a Hessian >= levenberg_marquardt (1e-2 for the triple's class, 1
for the double's) is within ~1e-6 of its solution; two such solves agree to 2e-6."""
import numpy as np

STEP_TOL = 2e-6
QP_CAP = 100


def lockstep_solve(first, second, pairs):
    def solve(x0, xg, ug, w=None):
        a = first(x0, xg, ug, w) if w is not None else first(x0, xg, ug)
        b = second(x0, xg, ug, w) if w is not None else second(x0, xg, ug)
        for j in range(x0.shape[0]):
            if a["status"][j] != b["status"][j]:
                k = "status"
            elif a["status"][j] != 0:
                k = "same"
            elif max(a["qp_iter"][j], b["qp_iter"][j]) >= QP_CAP:
                k = "cap" if min(a["qp_iter"][j], b["qp_iter"][j]) >= QP_CAP // 2 else "value"
            else:
                d = max(np.abs(a["u"][j] - b["u"][j]).max(), np.abs(a["x"][j] - b["x"][j]).max())
                k = "same" if d <= STEP_TOL else "value"
            pairs.append(k)
        return a
    return solve


def classify(pairs):
    counts = {k: pairs.count(k) for k in ("same", "cap", "status", "value")}
    print("closed-loop step pairs:", counts)
    assert counts["value"] == 0, counts
    assert counts["status"] <= max(2, len(pairs) // 100), counts   # reported and capped at 1 %
    return counts
