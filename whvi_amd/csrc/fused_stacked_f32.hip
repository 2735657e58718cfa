// whvi_amd/csrc/fused_stacked_f32.hip -- the rectangular fastfood layer in one launch, float: the instantiations of
// fused_shs_stacked_kernel (fused_stacked_fwd.hpp) and the ABI (include/whvi_hip.h: whvi_fused_shs_stacked_supported,
// whvi_fused_shs_stacked_f32).  The checks are abi.hip's.  Built like fused_f32.hip: -ffp-contract=off -fno-slp-vectorize.
#include "fused_stacked_fwd.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

WHVI_EXPORT int whvi_fused_shs_stacked_supported(int32_t log2d, int64_t n_blocks)
{
    return whvi::fused_stacked_supported(log2d, n_blocks) ? 1 : 0;
}

WHVI_EXPORT int whvi_fused_shs_stacked_f32(void *dst, const void *src, const void *a, const void *b, const void *c,
                                           int64_t n_blocks, int64_t n_samples, int64_t sample_stride, int32_t log2d,
                                           int32_t flags, void *stream)
{
    return whvi::fused_stacked_fwd_run<float, false>(dst, src, a, b, c, nullptr, n_blocks, n_samples, sample_stride, log2d, 0, 0,
                                                     flags, stream);
}
