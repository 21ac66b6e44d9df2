// solver_types.h - the solver's option and batch-input records, shared by its translation units (vboc_solver.hip,
// ft_chains.hip)
#pragma once

namespace vboc {

struct Opts {
  double tol_stat, tol_eq, tol_ineq, tol_comp;
  double qp_tol_stat, qp_tol_eq, qp_tol_comp;
  double alpha_min, alpha_red, lm, mu0, push, tau;
  int max_iter, qp_max_iter;
  // Cartesian path constraint hlh <= |tip(theta_k) - (hxc, hyc)|^2 <= huh on stages 0..N-1 (hc != 0;
  // vboc_set_path_constraint, VBOC/Cartesian constraints/doublependulum_class_fixedveldir.py:154-160)
  int hc;
  double hxc, hyc, hlh, huh;
};

struct Inputs {
  int B, nmax;
  const int* N;
  const double *xg, *ug, *p, *lbx, *ubx, *lbu, *ubu, *lbx0, *ubx0, *lbxe, *ubxe;
  int* status;
  double *xo, *uo, *cost;
  int *sqp_iter, *qp_iter;
  unsigned int* head;   // work-queue head
};

}  // namespace vboc
