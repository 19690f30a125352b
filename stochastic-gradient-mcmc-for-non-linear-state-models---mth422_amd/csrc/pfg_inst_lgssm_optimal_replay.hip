// Instantiation unit: every particle-filter kernel of (PFG_MODEL_LGSSM, PFG_KERNEL_OPTIMAL, PFG_RNG_REPLAY).
#include "pfg_launch.hpp"

namespace pfg_host {
template int launch_mkr<PFG_MODEL_LGSSM, PFG_KERNEL_OPTIMAL, PFG_RNG_REPLAY>(pfg_ctx *, const LaunchPlan &, int, const pfg_dev_problem *, hipStream_t);
}  // namespace pfg_host
