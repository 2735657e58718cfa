// whvi_amd/csrc/fused_stacked_layer_f32.hip -- the rectangular fastfood layer with its bias, its neighbouring ReLUs and its
// narrowing in one launch, float: the instantiations of fused_shs_stacked_layer_kernel (fused_stacked_fwd.hpp) and the ABI
// (include/whvi_hip.h: whvi_fused_shs_stacked_layer_supported, whvi_fused_shs_stacked_layer_f32).  The checks are abi.hip's.
// Built like fused_stacked_f32.hip: -ffp-contract=off -fno-slp-vectorize.
#include "fused_stacked_fwd.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

WHVI_EXPORT int whvi_fused_shs_stacked_layer_supported(int32_t log2d, int64_t n_blocks, int32_t has_bias)
{
    return whvi::fused_stacked_layer_supported(log2d, n_blocks, has_bias != 0) ? 1 : 0;
}

WHVI_EXPORT int whvi_fused_shs_stacked_layer_f32(void *dst, const void *src, const void *a, const void *b, const void *c,
                                                 const void *bias, int64_t n_blocks, int64_t n_samples, int64_t sample_stride,
                                                 int32_t log2d, int64_t n_cols, int64_t ld_dst, int32_t flags, void *stream)
{
    return whvi::fused_stacked_fwd_run<float, true>(dst, src, a, b, c, bias, n_blocks, n_samples, sample_stride, log2d, n_cols,
                                                    ld_dst, flags, stream);
}
