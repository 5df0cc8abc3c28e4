// bez_step_ws8.hip -- instantiations of the 8-role-wave fused step kernel (bez_kernel_ws8.h) without the actuator record (DF = false),
// through the header's launch ladder, and their launcher.
#include <hip/hip_runtime.h>

#include "bez_kernel_ws8.h"
#include "bez_launch.h"

namespace bez {

void launch_step_ws8(const Params& P, bool pre_post, bool dr, bool cleats, hipStream_t stream, bool ext) {
  w8::launch_ws8<false>(P, nullptr, pre_post, dr, cleats, ext, stream);
}

}  // namespace bez
