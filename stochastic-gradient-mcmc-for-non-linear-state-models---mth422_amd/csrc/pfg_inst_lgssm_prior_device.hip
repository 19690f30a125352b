// Instantiation unit: every particle-filter kernel of (PFG_MODEL_LGSSM, PFG_KERNEL_PRIOR, PFG_RNG_DEVICE).
#include "pfg_launch.hpp"

namespace pfg_host {
template int launch_mkr<PFG_MODEL_LGSSM, PFG_KERNEL_PRIOR, PFG_RNG_DEVICE>(pfg_ctx *, const LaunchPlan &, int, const pfg_dev_problem *, hipStream_t);
}  // namespace pfg_host
