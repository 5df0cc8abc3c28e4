// bez_step_ws8q_df.hip -- the 8-role-wave fused step kernel, the lane-group form (four lanes per env), compiled with the actuator record (BEZ_FLAG_DOF_FORCE:
// bez_kernels.h df_record) under a name of its own, and its launcher.  The same instantiations as bez_step_ws8q.hip, the spill-free default form included.
#include <hip/hip_runtime.h>

#define BEZ_DOF_FORCE 1
#define step_kernel step_kernel_df
#define step_kernel_ws8 step_kernel_ws8_df
#define BEZ_WS_SUB 4
#include "bez_kernel_ws8.h"
#include "bez_launch_df.h"

namespace bez {

template <bool PP>
static void launch_pp_df(const ParamsDF& P, bool dr, bool cleats, bool ext, dim3 grid, hipStream_t stream) {
  const dim3 block(w8q::WS_BLOCK);
  if (ext) {   // external wrenches (bez_sim_apply_body_forces): per-env parameter loads always on, null = defaults
    if (cleats) hipLaunchKernelGGL((w8q::step_kernel_ws8<PP, PP, true, true, true>), grid, block, 0, stream, P);
    else hipLaunchKernelGGL((w8q::step_kernel_ws8<PP, PP, true, false, true>), grid, block, 0, stream, P);
  } else if (cleats) hipLaunchKernelGGL((w8q::step_kernel_ws8<PP, PP, true, true>), grid, block, 0, stream, P);
  else if (dr) hipLaunchKernelGGL((w8q::step_kernel_ws8<PP, PP, true, false>), grid, block, 0, stream, P);
  else hipLaunchKernelGGL((w8q::step_kernel_ws8<PP, PP, false, false>), grid, block, 0, stream, P);
}

void launch_step_ws8q_df(const Params& P0, float* raw, bool pre_post, bool dr, bool cleats, hipStream_t stream, bool ext) {
  ParamsDF P;
  static_cast<Params&>(P) = P0;
  P.dof_force = raw;
  const dim3 grid((P.n + w8q::WS_ENVS - 1) / w8q::WS_ENVS);
  if (pre_post) launch_pp_df<true>(P, dr, cleats, ext, grid, stream);
  else launch_pp_df<false>(P, dr, cleats, ext, grid, stream);
}

}  // namespace bez
