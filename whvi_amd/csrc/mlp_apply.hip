// whvi_amd/csrc/mlp_apply.hip -- the predictive pass of a WHVI regression network (first layer, 1 .. 4 square layers, row
// dot) for all Monte-Carlo samples in one launch, f32.  ABI: include/whvi_hip.h (whvi_mlp_apply_f32, whvi_mlp_apply_supported).
#include "dispatch.hpp"
#include "mlp_apply.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

WHVI_EXPORT int whvi_mlp_apply_supported(int32_t first, int32_t n_mid, int32_t log2d)
{
    return whvi::mlp_supported(first, n_mid, log2d) ? 1 : 0;
}

WHVI_EXPORT int whvi_mlp_apply_f32(void *y, const void *x, int32_t first, const void *w_in, const void *b_in, int32_t n_mid,
                                   const void *s1, const void *s2, const void *u, const void *b_mid, int32_t mid_bias,
                                   const void *w_out, const void *b_out, int64_t S, int64_t B, int32_t log2d, int32_t relu,
                                   void *stream)
{
    return whvi::mlp_apply_dispatch(y, x, first, w_in, b_in, n_mid, s1, s2, u, b_mid, mid_bias, w_out, b_out, S, B, log2d, relu,
                                    stream);
}
