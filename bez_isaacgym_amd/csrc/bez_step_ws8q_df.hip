// bez_step_ws8q_df.hip -- the 8-role-wave fused step kernel, the lane-group form (four lanes per env), instantiated with the actuator record
// (BEZ_FLAG_DOF_FORCE: DF = true, entry point step_kernel_ws8_df; bez_kernels.h df_record), and its launcher.  The same instantiations as
// bez_step_ws8q.hip, the spill-free default form included.
#include <hip/hip_runtime.h>

// the entry point's switch and names (bez_kernels.h STEP_DF): the only use of the preprocessor for the record
#define BEZ_DOF_FORCE 1
#define step_kernel step_kernel_df
#define step_kernel_ws8 step_kernel_ws8_df
#define BEZ_WS_SUB 4
#include "bez_kernel_ws8.h"
#include "bez_launch.h"

namespace bez {

void launch_step_ws8q_df(const Params& P, float* raw, bool pre_post, bool dr, bool cleats, hipStream_t stream, bool ext) {
  w8q::launch_ws8<true>(P, raw, pre_post, dr, cleats, ext, stream);
}

}  // namespace bez
