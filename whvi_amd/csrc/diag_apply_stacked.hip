// whvi_amd/csrc/diag_apply_stacked.hip -- the batched pass of a reference-mode stacked layer of any width: all J diagonal
// blocks of every Monte-Carlo sample in one launch, f32.  ABI: include/whvi_hip.h (whvi_diag_apply_stacked_f32,
// whvi_diag_apply_stacked_supported).
#include "dispatch.hpp"
#include "diag_apply_stacked.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

namespace whvi {

static int diag_apply_stacked_dispatch(void *out, const void *x, const void *s1, const void *s2, const void *u, const void *bias,
                                       int64_t S, int64_t B, int32_t log2d, int64_t J, int64_t n_cols, int64_t ld_out,
                                       int32_t flags, void *stream)
{
    g_err[0] = 0;
    StackedDiagLaunch ln;
    const int rc = stacked_diag_check(ln, out, x, s1, s2, u, bias, S, B, log2d, J, n_cols, ld_out, flags);
    if (rc != WHVI_OK || ln.grid.x == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
#define WHVI_STACKED(C, NT)                                                                                     \
    do {                                                                                                        \
        note_launch<float>("diag_apply_stacked_kernel", C, (bool)NT);                                           \
        hipLaunchKernelGGL((diag_apply_stacked_kernel<float, C, NT>), ln.grid, dim3(256), ln.lds, st, (float *)out, \
                           (const float *)x, (const float *)s1, (const float *)s2, (const float *)u, (const float *)bias, \
                           (uint32_t)S, (uint32_t)B, (uint32_t)J, (uint32_t)log2d, (uint32_t)n_cols, ld_out, ln.opts,  \
                           ln.slab_rows, ln.n_slabs);                                                           \
    } while (0)
#define WHVI_CASE(C)                                                                                            \
    case C:                                                                                                     \
        if (ln.nt) WHVI_STACKED(C, true); else WHVI_STACKED(C, false);                                          \
        break;
    switch (stacked_diag_c(log2d)) {
        WHVI_CASE(1) WHVI_CASE(2) WHVI_CASE(4) WHVI_CASE(8) WHVI_CASE(16)
    default: break;
    }
#undef WHVI_CASE
#undef WHVI_STACKED
    return after_launch("diag_apply_stacked");
}

}  // namespace whvi

WHVI_EXPORT int whvi_diag_apply_stacked_supported(int32_t log2d, int64_t n_blocks)
{
    return whvi::stacked_diag_supported(log2d, n_blocks) ? 1 : 0;
}

WHVI_EXPORT int whvi_diag_apply_stacked_f32(void *out, const void *x, const void *s1, const void *s2, const void *u,
                                            const void *bias, int64_t S, int64_t B, int32_t log2d, int64_t n_blocks,
                                            int64_t n_cols, int64_t ld_out, int32_t flags, void *stream)
{
    return whvi::diag_apply_stacked_dispatch(out, x, s1, s2, u, bias, S, B, log2d, n_blocks, n_cols, ld_out, flags, stream);
}
