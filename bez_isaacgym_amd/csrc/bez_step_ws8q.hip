// bez_step_ws8q.hip -- the lane-group form of the 8-role-wave fused step kernel: bez_kernel_ws8.h compiled with four lanes per env
// (namespace w8q: 16 envs per workgroup, 256 workgroups at 4096 envs), selected per sim with BEZ_SIM_KERNEL=ws8q.  The instantiations
// without the actuator record (DF = false), through the header's launch ladder.
#include <hip/hip_runtime.h>

#define BEZ_WS_SUB 4
#include "bez_kernel_ws8.h"
#include "bez_launch.h"

namespace bez {

void launch_step_ws8q(const Params& P, bool pre_post, bool dr, bool cleats, hipStream_t stream, bool ext) {
  w8q::launch_ws8<false>(P, nullptr, pre_post, dr, cleats, ext, stream);
}

}  // namespace bez
