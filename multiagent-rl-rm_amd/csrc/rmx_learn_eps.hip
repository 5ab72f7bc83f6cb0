// rmx_learn_eps.hip — learn_step_kernel's instantiations with a per-learner epsilon schedule (rmx_learn_eps_bind) and
// their launcher, launch_learn_step_eps: rmx_learn.hip compiled once more, as a translation unit of its own, so that
// the two sets of kernels build side by side and the kernels without a schedule stay exactly as they were.
#define RMX_LEARN_EPS_TU 1
#include "rmx_learn.hip"
