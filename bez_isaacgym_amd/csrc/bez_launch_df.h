// bez_launch_df.h -- launchers of the step kernels that record the actuator quantities (BEZ_FLAG_DOF_FORCE): the kernels of bez_launch.h,
// compiled a second time with BEZ_DOF_FORCE defined, in translation units of their own (bez_step_ws8_df.hip, bez_step_ws8q_df.hip,
// bez_step_lane_df.hip) and under names of their own, so that the kernels a sim without the flag launches are untouched.  `raw`: the
// sim's raw actuator buffer, [substep][quantity][dof][env] (bez_kernels.h df_record).  Physics launches only (the lane kernel's PRE-only /
// POST-only forms record nothing and stay in bez_step_lane.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "bez_kernels.h"

namespace bez {
void launch_step_ws8_df(const Params& P, float* raw, bool pre_post, bool dr, bool cleats, hipStream_t stream, bool ext);
void launch_step_ws8q_df(const Params& P, float* raw, bool pre_post, bool dr, bool cleats, hipStream_t stream, bool ext);
void launch_step_lane_df(const Params& P, float* raw, bool pre_post, bool dr, bool cleats, hipStream_t stream, bool ext);
}  // namespace bez
