// whvi_amd/csrc/diag_apply_stacked_bwd.hip -- backward of the stacked layer's one-launch pass on the blocks' diagonals, f32.
// ABI: include/whvi_hip.h (whvi_diag_apply_stacked_bwd_f32, whvi_diag_apply_stacked_bwd_supported,
// whvi_diag_apply_stacked_bwd_slabs).
#include "dispatch.hpp"
#include "diag_apply_stacked_bwd.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

namespace whvi {

static int diag_apply_stacked_bwd_dispatch(void *grad_x, void *out, void *part, const void *g, const void *x, const void *s1,
                                           const void *s2, const void *u, const void *bias, int64_t S, int64_t B, int32_t log2d,
                                           int64_t J, int64_t n_cols, int64_t ld_g, int64_t n_slabs, int32_t flags, void *stream)
{
    g_err[0] = 0;
    StackedDiagBwdLaunch ln;
    int rc = stacked_diag_bwd_check(ln, grad_x, out, part, g, x, s1, s2, u, bias, S, B, log2d, J, n_cols, ld_g, n_slabs, flags);
    if (rc != WHVI_OK || ln.grid.x == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
#define WHVI_SDB(C, NT, GX)                                                                                     \
    do {                                                                                                        \
        note_launch<float>("stacked_diag_bwd_kernel", C, (bool)NT, (bool)GX);                                   \
        hipLaunchKernelGGL((stacked_diag_bwd_kernel<float, C, NT, GX>), ln.grid, dim3(256), ln.lds, st, (float *)grad_x, \
                           (float *)part, (const float *)g, (const float *)x, (const float *)s1, (const float *)s2, \
                           (const float *)u, (const float *)bias, (uint32_t)S, (uint32_t)B, (uint32_t)J, (uint32_t)log2d, \
                           (uint32_t)n_cols, ld_g, ln.opts, ln.slab_rows, (uint32_t)n_slabs);                   \
    } while (0)
#define WHVI_CASE(C)                                                                                            \
    case C:                                                                                                     \
        if (grad_x == nullptr) WHVI_SDB(C, false, false);                                                       \
        else if (ln.nt) WHVI_SDB(C, true, true);                                                                \
        else WHVI_SDB(C, false, true);                                                                          \
        break;
    switch (stacked_diag_bwd_cpt(J << (log2d - 2))) {
        WHVI_CASE(1) WHVI_CASE(2) WHVI_CASE(4) WHVI_CASE(8)
    default: break;
    }
#undef WHVI_CASE
#undef WHVI_SDB
    rc = after_launch("diag_apply_stacked_bwd");
    if (rc != WHVI_OK) return rc;
    const uint32_t JD = (uint32_t)(J << log2d);
    hipLaunchKernelGGL((stacked_diag_bwd_finish_kernel<float>), dim3((JD + 255) / 256, (unsigned)S), dim3(256), 0, st, (float *)out,
                       (const float *)part, (const float *)s1, (const float *)s2, (const float *)u, (uint32_t)n_slabs,
                       (uint32_t)log2d, (uint32_t)J, (uint32_t)S, (uint32_t)n_cols, (flags & WHVI_DIAG_MEAN_PLUS) ? 1u : 0u);
    return after_launch("diag_apply_stacked_bwd (finish)");
}

}  // namespace whvi

WHVI_EXPORT int whvi_diag_apply_stacked_bwd_supported(int32_t log2d, int64_t n_blocks)
{
    return whvi::stacked_diag_bwd_supported(log2d, n_blocks) ? 1 : 0;
}

WHVI_EXPORT int64_t whvi_diag_apply_stacked_bwd_slabs(int64_t S, int64_t B, int32_t log2d, int64_t n_blocks, int64_t n_cols)
{
    (void)n_cols;      // (the slab count follows the row's J D columns: the geometry does not change with the narrowing)
    return whvi::stacked_diag_bwd_slabs(S, B, log2d, n_blocks);
}

WHVI_EXPORT int whvi_diag_apply_stacked_bwd_f32(void *grad_x, void *out, void *part, const void *g, const void *x, const void *s1,
                                                const void *s2, const void *u, const void *bias, int64_t S, int64_t B,
                                                int32_t log2d, int64_t n_blocks, int64_t n_cols, int64_t ld_g, int64_t n_slabs,
                                                int32_t flags, void *stream)
{
    return whvi::diag_apply_stacked_bwd_dispatch(grad_x, out, part, g, x, s1, s2, u, bias, S, B, log2d, n_blocks, n_cols, ld_g,
                                                 n_slabs, flags, stream);
}
