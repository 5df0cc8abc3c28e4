// bez_step_lane_df.hip -- the one-env-per-lane step kernel (bez_kernels.h) compiled with the actuator record (BEZ_FLAG_DOF_FORCE) and its
// launcher: the physics-carrying forms only (the whole control step, the physics alone).
#include <hip/hip_runtime.h>

#define BEZ_DOF_FORCE 1
#define step_kernel step_kernel_df
#include "bez_launch_df.h"

namespace bez {

template <bool PP>
static void launch_pp_df(const ParamsDF& P, bool dr, bool cleats, bool ext, hipStream_t stream) {
  const dim3 grid((P.n + BLOCK - 1) / BLOCK), block(BLOCK);
  if (ext) {   // external wrenches (bez_sim_apply_body_forces): per-env parameter loads always on, null = defaults
    if (cleats) hipLaunchKernelGGL((step_kernel<PP, true, PP, true, true, true>), grid, block, 0, stream, P);
    else hipLaunchKernelGGL((step_kernel<PP, true, PP, true, false, true>), grid, block, 0, stream, P);
  } else if (cleats) hipLaunchKernelGGL((step_kernel<PP, true, PP, true, true>), grid, block, 0, stream, P);
  else if (dr) hipLaunchKernelGGL((step_kernel<PP, true, PP, true, false>), grid, block, 0, stream, P);
  else hipLaunchKernelGGL((step_kernel<PP, true, PP, false, false>), grid, block, 0, stream, P);
}

void launch_step_lane_df(const Params& P0, float* raw, bool pre_post, bool dr, bool cleats, hipStream_t stream, bool ext) {
  ParamsDF P;
  static_cast<Params&>(P) = P0;
  P.dof_force = raw;
  if (pre_post) launch_pp_df<true>(P, dr, cleats, ext, stream);
  else launch_pp_df<false>(P, dr, cleats, ext, stream);
}

}  // namespace bez
