// whvi_amd/csrc/fused_stacked_f16.hip -- the rectangular fastfood layer in one launch, __half activations with float32 scale
// vectors: the instantiations of fused_stacked16_kernel<__half, ...> (fused_stacked_fwd.hpp; one translation unit per dtype so
// the library builds in parallel).  The checks are abi.hip's.  ABI: include/whvi_hip.h.  Built like fused_bwd_f16.hip:
// -ffp-contract=off -fno-slp-vectorize.
#include "fused_stacked_fwd.hpp"

extern "C" __attribute__((visibility("default")))
int whvi_fused_shs_stacked_f16(void *dst, const void *src, const void *a, const void *b, const void *c, int64_t n_blocks,
                               int64_t n_samples, int64_t sample_stride, int32_t log2d, int32_t flags, void *stream)
{
    return whvi::fused_stacked_fwd_run<__half, false>(dst, src, a, b, c, nullptr, n_blocks, n_samples, sample_stride, log2d, 0, 0,
                                                      flags, stream);
}
