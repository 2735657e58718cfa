// whvi_amd/csrc/fused_stacked_f32.hip -- the rectangular fastfood layer in one launch, float: the instantiations of
// fused_shs_stacked_kernel (fused_stacked.hpp), the argument checks and the ABI (include/whvi_hip.h:
// whvi_fused_shs_stacked_supported, whvi_fused_shs_stacked_f32).  Built like fused_f32.hip: -ffp-contract=off
// -fno-slp-vectorize.
#include "dispatch.hpp"
#include "fused_stacked.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

namespace whvi {

// Every argument check of whvi_fused_shs_stacked_f32, before any device call.  WHVI_OK with launch = false: nothing to launch.
static int fused_stacked_check(FusedStackedArgs &r, bool &launch, void *dst, const void *src, const void *a, const void *b,
                               const void *c, int64_t J, int64_t S, int64_t stride, int32_t log2d, int32_t flags)
{
    g_err[0] = 0;
    launch = false;
    if (flags & ~WHVI_FUSED_SRC_SHARED)
        return fail(WHVI_ERR_ARG, "whvi_fused_shs_stacked: unknown fused flags%s 0x%llx (0 or the shared-source flag)", "", flags);
    if (J < 0 || S < 0 || stride < 0) return fail(WHVI_ERR_ARG, "whvi_fused_shs_stacked: negative size%s", "");
    if (log2d < FUSED_STACKED_MIN_LOG2D || log2d > FUSED_STACKED_MAX_LOG2D)
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked: log2(D)%s = %lld is outside the supported range [6, %lld]", "", log2d,
                    FUSED_STACKED_MAX_LOG2D);
    if (!fused_stacked_supported(log2d, J))
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked: %s%lld blocks need 12 D bytes of LDS each, at most %lld fit 64 KiB", "", J,
                    FUSED_STACKED_LDS_BYTES / ((int64_t)12 << log2d));
    if (S == 0 || stride == 0) return WHVI_OK;
    if (!dst || !src || !a || !b || !c) return fail(WHVI_ERR_ARG, "whvi_fused_shs_stacked: null pointer%s", "");
    if (S >= ((int64_t)1 << 32) / stride)
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked: rows are indexed with 32 bits%s", "");
    if (((uintptr_t)dst | (uintptr_t)src | (uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15)
        return fail(WHVI_ERR_ALIGN, "whvi_fused_shs_stacked: a pointer%s is not 16-byte aligned", "");
    const FusedBwdGeom geom = fused_bwd_geom(S, stride, log2d);
    if (S * geom.n_slabs >= ((int64_t)1 << 31)) return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked: too many blocks%s", "");
    const int64_t row_bytes = (int64_t)4 << log2d, rows = S * stride;
    const bool shared = (flags & WHVI_FUSED_SRC_SHARED) != 0;
    const struct { const void *p; int64_t bytes; } ins[] = {
        {src, (shared ? stride : rows) * row_bytes}, {a, J * row_bytes}, {b, J * S * row_bytes}, {c, J * row_bytes}};
    for (const auto &t : ins)
        if (ranges_overlap(dst, rows * J * row_bytes, t.p, t.bytes))
            return fail(WHVI_ERR_OVERLAP, "whvi_fused_shs_stacked: dst overlaps an input%s", "");
    r.dst = dst, r.src = src, r.a = a, r.b = b, r.c = c;
    r.n_blocks = J, r.n_samples = S, r.sample_stride = stride, r.log2d = log2d, r.src_shared = shared, r.geom = geom;
    // the streamed bytes: the J output segments, and the source unless it is shared
    r.nt = rows * row_bytes * (J + (shared ? 0 : 1)) > NT_MIN_BYTES;
    launch = true;
    return WHVI_OK;
}

}  // namespace whvi

using namespace whvi;

WHVI_EXPORT int whvi_fused_shs_stacked_supported(int32_t log2d, int64_t n_blocks)
{
    return fused_stacked_supported(log2d, n_blocks) ? 1 : 0;
}

WHVI_EXPORT int whvi_fused_shs_stacked_f32(void *dst, const void *src, const void *a, const void *b, const void *c,
                                           int64_t n_blocks, int64_t n_samples, int64_t sample_stride, int32_t log2d,
                                           int32_t flags, void *stream)
{
    FusedStackedArgs r;
    bool launch = false;
    const int rc = fused_stacked_check(r, launch, dst, src, a, b, c, n_blocks, n_samples, sample_stride, log2d, flags);
    if (rc != WHVI_OK || !launch) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (log2d) {
    case 6: fused_stacked_launch_one<float, 6>(r, st); break;
    case 7: fused_stacked_launch_one<float, 7>(r, st); break;
    case 8: fused_stacked_launch_one<float, 8>(r, st); break;
    case 9: fused_stacked_launch_one<float, 9>(r, st); break;
    case 10: fused_stacked_launch_one<float, 10>(r, st); break;
    default: fused_stacked_launch_one<float, 11>(r, st); break;
    }
    return after_launch("fused_shs_stacked");
}
