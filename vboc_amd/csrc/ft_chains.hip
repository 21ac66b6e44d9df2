// ft_chains.hip - the tracking solver of ft.h with per-problem references (k_ftr<1>, k_ftr<2>, k_ftr<3>): the pendulum and
// the double pendulum (AL's labelling OCPs of AL/pendulum_class_al.py and AL/doublependulum_class_al.py, the 2dof Safe MPC
// of VBOC/Safe MPC/*/doublependulum_class_fixedveldir.py), and the triple when a batch passes yref_b / yref_e_b.
// A translation unit of its own: device code added to vboc_solver.hip moves the code laid out after it, and with it
// the PC-relative call offsets that the arm's kernels are pinned with (tests/test_isa_guard.py).
#include <hip/hip_runtime.h>

#include "solver_types.h"
#include "ft.h"

namespace vboc {

int launch_ft_chains(int nq, unsigned groups, hipStream_t st, const Opts& o, const Inputs& in, double* regions,
                     long long rd, unsigned* head, const MpcArgsY& mp) {
  switch (nq) {
    case 1: hipLaunchKernelGGL((k_ftr<1>), dim3(groups), dim3(64), 0, st, o, in, regions, rd, head, mp); break;
    case 2: hipLaunchKernelGGL((k_ftr<2>), dim3(groups), dim3(64), 0, st, o, in, regions, rd, head, mp); break;
    case 3: hipLaunchKernelGGL((k_ftr<3>), dim3(groups), dim3(64), 0, st, o, in, regions, rd, head, mp); break;
    default: return -2;
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace vboc
