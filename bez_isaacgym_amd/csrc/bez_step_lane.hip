// bez_step_lane.hip -- instantiations of the one-env-per-lane step kernel (bez_kernels.h) without the actuator record (DF = false) and
// their launcher: the physics-carrying forms through the launch ladder of bez_kernels.h, the split PRE-only / POST-only forms here.
#include <hip/hip_runtime.h>

#include "bez_launch.h"

namespace bez {

template <bool PRE, bool POST>
static void launch_split(const Params& P, bool dr, bool cleats, hipStream_t stream) {
  const dim3 grid((P.n + BLOCK - 1) / BLOCK), block(BLOCK);
  if (cleats) hipLaunchKernelGGL((step_kernel<PRE, false, POST, true, true>), grid, block, 0, stream, P);
  else if (dr) hipLaunchKernelGGL((step_kernel<PRE, false, POST, true, false>), grid, block, 0, stream, P);
  else hipLaunchKernelGGL((step_kernel<PRE, false, POST, false, false>), grid, block, 0, stream, P);
}

void launch_step_lane(const Params& P, bool pre, bool sim, bool post, bool dr, bool cleats, hipStream_t stream, bool ext) {
  if (pre && sim && post) launch_lane<false>(P, nullptr, true, dr, cleats, ext, stream);
  else if (pre && !sim && !post) launch_split<true, false>(P, dr, cleats, stream);
  else if (!pre && sim && !post) launch_lane<false>(P, nullptr, false, dr, cleats, ext, stream);
  else if (!pre && !sim && post) launch_split<false, true>(P, dr, cleats, stream);
}

}  // namespace bez
