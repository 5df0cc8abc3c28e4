// bez_launch.h -- the step kernels are compiled in their own translation units (bez_step_ws8.hip, bez_step_ws8q.hip, bez_step_lane.hip
// and, with the actuator record, bez_step_ws8_df.hip, bez_step_ws8q_df.hip, bez_step_lane_df.hip) so that the heavy units build side by
// side; bez_sim.hip (the C ABI) launches them through these functions.
// Instantiations: the default asset keeps a specialisation without the per-env parameter loads (the benchmark path); the
// cleats asset is always built with them (null pointers = defaults), which halves the number of variants.  `ext`: the sim has called
// bez_sim_apply_body_forces -- the instantiations that read the pending external wrenches (built with the per-env parameter loads only).
#pragma once
#include <hip/hip_runtime.h>

#include "bez_kernels.h"

namespace bez {
// fused wave-specialised step with 8 role waves per 64 envs (bez_kernel_ws8.h): (PRE, POST) = (pre, pre) -- the whole control
// step, or the physics alone
void launch_step_ws8(const Params& P, bool pre_post, bool dr, bool cleats, hipStream_t stream, bool ext = false);
// the same kernel in its lane-group form (bez_step_ws8q.hip: four lanes per env, 16 envs per workgroup)
void launch_step_ws8q(const Params& P, bool pre_post, bool dr, bool cleats, hipStream_t stream, bool ext = false);
// one-env-per-lane kernel: split entry points (PRE / SIM / POST alone), the obs-only pass and the A/B reference of the fused step
void launch_step_lane(const Params& P, bool pre, bool sim, bool post, bool dr, bool cleats, hipStream_t stream, bool ext = false);
// The same kernels with the actuator record (BEZ_FLAG_DOF_FORCE): the kernel templates instantiated with DF = true behind entry points of
// their own, so that the kernels a sim without the flag launches are untouched.  `raw`: the sim's raw actuator buffer,
// [substep][quantity][dof][env] (bez_kernels.h df_record).  Physics launches only (the lane kernel's PRE-only / POST-only forms record
// nothing).
void launch_step_ws8_df(const Params& P, float* raw, bool pre_post, bool dr, bool cleats, hipStream_t stream, bool ext);
void launch_step_ws8q_df(const Params& P, float* raw, bool pre_post, bool dr, bool cleats, hipStream_t stream, bool ext);
void launch_step_lane_df(const Params& P, float* raw, bool pre_post, bool dr, bool cleats, hipStream_t stream, bool ext);
constexpr int WS_ENVS_PER_GROUP = 64;
}  // namespace bez
