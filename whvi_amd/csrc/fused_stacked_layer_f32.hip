// whvi_amd/csrc/fused_stacked_layer_f32.hip -- the rectangular fastfood layer with its bias, its neighbouring ReLUs and its
// narrowing in one launch, float: the instantiations of fused_shs_stacked_layer_kernel (fused_stacked_layer.hpp), the argument
// checks and the ABI (include/whvi_hip.h: whvi_fused_shs_stacked_layer_supported, whvi_fused_shs_stacked_layer_f32).  Built like
// fused_stacked_f32.hip: -ffp-contract=off -fno-slp-vectorize.
#include "dispatch.hpp"
#include "fused_stacked_layer.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

namespace whvi {

constexpr int32_t FUSED_STACKED_LAYER_FLAGS = WHVI_FUSED_SRC_SHARED | WHVI_FUSED_RELU_IN | WHVI_FUSED_RELU_OUT;

// Every argument check of whvi_fused_shs_stacked_layer_f32, before any device call, in fused_stacked_check's order.  WHVI_OK
// with launch = false: nothing to launch.
static int fused_stacked_layer_check(FusedStackedLayerArgs &r, bool &launch, void *dst, const void *src, const void *a,
                                     const void *b, const void *c, const void *bias, int64_t J, int64_t S, int64_t stride,
                                     int32_t log2d, int64_t n_cols, int64_t ld_dst, int32_t flags)
{
    g_err[0] = 0;
    launch = false;
    if (flags & ~FUSED_STACKED_LAYER_FLAGS)
        return fail(WHVI_ERR_ARG, "whvi_fused_shs_stacked_layer: unknown fused flags%s 0x%llx (shared source, ReLU in, ReLU out)", "",
                    flags);
    if (J < 0 || S < 0 || stride < 0 || n_cols < 0 || ld_dst < 0)
        return fail(WHVI_ERR_ARG, "whvi_fused_shs_stacked_layer: negative size%s", "");
    if (log2d < FUSED_STACKED_MIN_LOG2D || log2d > FUSED_STACKED_MAX_LOG2D)
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer: log2(D)%s = %lld is outside the supported range [6, %lld]", "",
                    log2d, FUSED_STACKED_MAX_LOG2D);
    const int64_t per_block = (int64_t)(bias ? 16 : 12) << log2d;
    if (!fused_stacked_layer_supported(log2d, J, bias != nullptr))
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer: %s%lld blocks do not fit 64 KiB of LDS (at most %lld with these operands)",
                    "", J, FUSED_STACKED_LDS_BYTES / per_block);
    if ((n_cols | ld_dst) & 3)
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer: n_cols%s = %lld and ld_dst = %lld must be multiples of 4", "", n_cols,
                    ld_dst);
    if (n_cols <= ((J - 1) << log2d) || n_cols > (J << log2d))
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer: n_cols%s = %lld must end in the last of the %lld blocks", "", n_cols, J);
    if (ld_dst < n_cols || ld_dst >= ((int64_t)1 << 32))
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer: ld_dst%s = %lld is below n_cols = %lld (or beyond 32 bits)", "", ld_dst,
                    n_cols);
    if (S == 0 || stride == 0) return WHVI_OK;
    if (!dst || !src || !a || !b || !c) return fail(WHVI_ERR_ARG, "whvi_fused_shs_stacked_layer: null pointer%s", "");
    if (S >= ((int64_t)1 << 32) / stride)
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer: rows are indexed with 32 bits%s", "");
    if (((uintptr_t)dst | (uintptr_t)src | (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)bias) & 15)
        return fail(WHVI_ERR_ALIGN, "whvi_fused_shs_stacked_layer: a pointer%s is not 16-byte aligned", "");
    const FusedBwdGeom geom = fused_bwd_geom(S, stride, log2d);
    if (S * geom.n_slabs >= ((int64_t)1 << 31)) return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer: too many blocks%s", "");
    const int64_t row_bytes = (int64_t)4 << log2d, rows = S * stride;
    const bool shared = (flags & WHVI_FUSED_SRC_SHARED) != 0;
    const struct { const void *p; int64_t bytes; } ins[] = {
        {src, (shared ? stride : rows) * row_bytes}, {a, J * row_bytes}, {b, J * S * row_bytes}, {c, J * row_bytes},
        {bias, bias ? J * row_bytes : 0}};
    for (const auto &t : ins)
        if (t.bytes && ranges_overlap(dst, rows * ld_dst * 4, t.p, t.bytes))
            return fail(WHVI_ERR_OVERLAP, "whvi_fused_shs_stacked_layer: dst overlaps an input%s", "");
    r.dst = dst, r.src = src, r.a = a, r.b = b, r.c = c, r.bias = bias;
    r.n_blocks = J, r.n_samples = S, r.sample_stride = stride, r.n_cols = n_cols, r.ld_dst = ld_dst, r.log2d = log2d;
    r.opts = ((flags & WHVI_FUSED_RELU_IN) ? STACKED_OPT_RELU_IN : 0u) | ((flags & WHVI_FUSED_RELU_OUT) ? STACKED_OPT_RELU_OUT : 0u) |
             (bias ? STACKED_OPT_BIAS : 0u);
    r.src_shared = shared, r.geom = geom;
    // the streamed bytes: the n_cols written columns, and the source unless it is shared
    r.nt = rows * (4 * n_cols + (shared ? 0 : row_bytes)) > NT_MIN_BYTES;
    launch = true;
    return WHVI_OK;
}

}  // namespace whvi

using namespace whvi;

WHVI_EXPORT int whvi_fused_shs_stacked_layer_supported(int32_t log2d, int64_t n_blocks, int32_t has_bias)
{
    return fused_stacked_layer_supported(log2d, n_blocks, has_bias != 0) ? 1 : 0;
}

WHVI_EXPORT int whvi_fused_shs_stacked_layer_f32(void *dst, const void *src, const void *a, const void *b, const void *c,
                                                 const void *bias, int64_t n_blocks, int64_t n_samples, int64_t sample_stride,
                                                 int32_t log2d, int64_t n_cols, int64_t ld_dst, int32_t flags, void *stream)
{
    FusedStackedLayerArgs r;
    bool launch = false;
    const int rc = fused_stacked_layer_check(r, launch, dst, src, a, b, c, bias, n_blocks, n_samples, sample_stride, log2d, n_cols,
                                             ld_dst, flags);
    if (rc != WHVI_OK || !launch) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (log2d) {
    case 6: fused_stacked_layer_launch_one<float, 6>(r, st); break;
    case 7: fused_stacked_layer_launch_one<float, 7>(r, st); break;
    case 8: fused_stacked_layer_launch_one<float, 8>(r, st); break;
    case 9: fused_stacked_layer_launch_one<float, 9>(r, st); break;
    case 10: fused_stacked_layer_launch_one<float, 10>(r, st); break;
    default: fused_stacked_layer_launch_one<float, 11>(r, st); break;
    }
    return after_launch("fused_shs_stacked_layer");
}
