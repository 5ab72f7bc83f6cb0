// rmx_learn_run_eps.hip — learn_run_kernel's instantiations with a per-learner epsilon schedule (rmx_learn_eps_bind)
// and their launcher, launch_learn_run_eps: rmx_learn_run.hip compiled once more, as rmx_learn_eps.hip does it for the
// single step.
#define RMX_LEARN_EPS_TU 1
#include "rmx_learn_run.hip"
