// whvi_amd/csrc/fused_stacked_layer_f16.hip -- the rectangular fastfood layer with its bias, its neighbouring ReLUs and its
// narrowing in one launch, __half activations with float32 scale vectors and bias: the instantiations of
// fused_stacked16_layer_kernel<__half, ...> (fused_stacked_fwd.hpp; one translation unit per dtype so the library builds in
// parallel).  The checks are abi.hip's.  ABI: include/whvi_hip.h.  Built like fused_stacked_f16.hip: -ffp-contract=off
// -fno-slp-vectorize.
#include "fused_stacked_fwd.hpp"

extern "C" __attribute__((visibility("default")))
int whvi_fused_shs_stacked_layer_f16(void *dst, const void *src, const void *a, const void *b, const void *c, const void *bias,
                                     int64_t n_blocks, int64_t n_samples, int64_t sample_stride, int32_t log2d, int64_t n_cols,
                                     int64_t ld_dst, int32_t flags, void *stream)
{
    return whvi::fused_stacked_fwd_run<__half, true>(dst, src, a, b, c, bias, n_blocks, n_samples, sample_stride, log2d, n_cols,
                                                     ld_dst, flags, stream);
}
