// whvi_amd/csrc/mlp_fastfood_smooth_apply_bwd.hip -- the sigmoid and tanh instantiations of mlp_fastfood_apply_bwd_kernel
// (mlp_fastfood_apply_bwd.hpp), in a translation unit of their own so that they compile beside the ReLU ones.  The ABI and the
// finishing launch are in mlp_fastfood_apply_bwd.hip.
#include "dispatch.hpp"
#include "mlp_fastfood_apply_bwd.hpp"

namespace whvi {

WHVI_MLP_FF_BWD_DEFINE(mlp_ff_bwd_launch_sigmoid, WHVI_MLP_ACT_SIGMOID)
WHVI_MLP_FF_BWD_DEFINE(mlp_ff_bwd_launch_tanh, WHVI_MLP_ACT_TANH)

}  // namespace whvi
