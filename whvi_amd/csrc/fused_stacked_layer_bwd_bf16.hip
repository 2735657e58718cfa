// whvi_amd/csrc/fused_stacked_layer_bwd_bf16.hip -- one-launch backward of the rectangular fastfood layer with its epilogue,
// __hip_bfloat16 activations with float32 scale vectors, gradients and workspace: the instantiations of
// fused_layer_bwd16_kernel<__hip_bfloat16, ...> (fused_stacked_layer_bwd16.hpp; one translation unit per dtype so the library
// builds in parallel).  The checks and the finishing launch are fused_stacked_layer_bwd_f16.hip's.  ABI: include/whvi_hip.h.
// Built like fused_stacked_bwd_f16.hip: -ffp-contract=off -fno-slp-vectorize.
#include "fused_stacked_layer_bwd16.hpp"

extern "C" __attribute__((visibility("default")))
int whvi_fused_shs_stacked_layer_bwd_bf16(void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *grad_bias, void *work,
                                          const void *grad_y, const void *y, const void *x, const void *a, const void *b,
                                          const void *c, int64_t n_blocks, int64_t n_samples, int64_t sample_stride, int32_t log2d,
                                          int64_t n_cols, int64_t ld, int32_t flags, void *stream)
{
    return whvi::fused_layer_bwd16_run<__hip_bfloat16>(grad_x, grad_a, grad_b, grad_c, grad_bias, work, grad_y, y, x, a, b, c,
                                                       n_blocks, n_samples, sample_stride, log2d, n_cols, ld, flags, stream);
}
