// bez_step_lane_df.hip -- instantiations of the one-env-per-lane step kernel (bez_kernels.h) with the actuator record (BEZ_FLAG_DOF_FORCE:
// DF = true, entry point step_kernel_df) and their launcher: the physics-carrying forms only (the whole control step, the physics alone).
#include <hip/hip_runtime.h>

// the entry point's switch and names (bez_kernels.h STEP_DF): the only use of the preprocessor for the record
#define BEZ_DOF_FORCE 1
#define step_kernel step_kernel_df
#include "bez_launch.h"

namespace bez {

void launch_step_lane_df(const Params& P, float* raw, bool pre_post, bool dr, bool cleats, hipStream_t stream, bool ext) {
  launch_lane<true>(P, raw, pre_post, dr, cleats, ext, stream);
}

}  // namespace bez
