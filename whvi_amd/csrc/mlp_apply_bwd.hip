// whvi_amd/csrc/mlp_apply_bwd.hip -- backward of the one-launch predictive pass of a WHVI regression network, f32.
// ABI: include/whvi_hip.h (whvi_mlp_apply_bwd_f32, whvi_mlp_apply_bwd_supported, whvi_mlp_apply_bwd_workspace).
#include "dispatch.hpp"
#include "mlp_apply_bwd.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

WHVI_EXPORT int whvi_mlp_apply_bwd_supported(int32_t first, int32_t n_mid, int32_t log2d)
{
    return whvi::mlp_bwd_supported(first, n_mid, log2d) ? 1 : 0;
}

WHVI_EXPORT int64_t whvi_mlp_apply_bwd_workspace(int64_t S, int64_t B, int32_t first, int32_t n_mid, int32_t log2d)
{
    return whvi::mlp_apply_bwd_workspace(S, B, first, n_mid, log2d);
}

WHVI_EXPORT int whvi_mlp_apply_bwd_f32(void *grad_w_in, void *grad_w_mid, void *grad_w_out, void *grad_b, void *grad_x,
                                       void *work, int64_t work_floats, const void *g, const void *x, int32_t first,
                                       const void *w_in, const void *b_in, int32_t n_mid, const void *s1, const void *s2,
                                       const void *u, const void *b_mid, int32_t mid_bias, const void *w_out, int64_t S,
                                       int64_t B, int32_t log2d, int32_t relu, void *stream)
{
    return whvi::mlp_apply_bwd_dispatch(grad_w_in, grad_w_mid, grad_w_out, grad_b, grad_x, work, work_floats, g, x, first, w_in,
                                        b_in, n_mid, s1, s2, u, b_mid, mid_bias, w_out, S, B, log2d, relu, stream);
}
