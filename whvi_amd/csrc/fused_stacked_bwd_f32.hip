// whvi_amd/csrc/fused_stacked_bwd_f32.hip -- one-launch backward of the rectangular fastfood layer, float: the instantiations of
// fused_shs_stacked_bwd_kernel (fused_stacked_bwd.hpp), the finishing launch, the argument checks and the ABI
// (include/whvi_hip.h: whvi_fused_shs_stacked_bwd_supported, whvi_fused_shs_stacked_bwd_workspace,
// whvi_fused_shs_stacked_bwd_f32).  Built like fused_f32.hip: -ffp-contract=off -fno-slp-vectorize.
#include "dispatch.hpp"
#include "fused_stacked_bwd.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

namespace whvi {

// Slots of [j][a | b | c][D] in ascending block order.  Per j, (S + 2) D threads as fused_shs_bwd_finish_kernel has them: thread
// t < S D: grad_b[j][s][n] over the n_slabs blocks of sample s; the next D: grad_a[j][n] over all S n_slabs blocks; the last D:
// grad_c[j][n].  Eight loads in flight, added in order.
__global__ void __launch_bounds__(256)
fused_shs_stacked_bwd_finish_kernel(float *__restrict__ ga, float *__restrict__ gb, float *__restrict__ gc,
                                    const float *__restrict__ part, uint32_t J, uint32_t S, uint32_t n_slabs, uint32_t log2d)
{
    const uint32_t D = 1u << log2d;
    const size_t ps = (size_t)3 * J << log2d;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= J * (S + 2) * D) return;
    const uint32_t n = t & (D - 1), jrow = t >> log2d, j = jrow / (S + 2), row = jrow - j * (S + 2);
    const float *p = part + ((size_t)3 * j << log2d) + n;
    float *dst;
    uint32_t count;
    if (row < S) p += (size_t)row * n_slabs * ps + D, dst = gb + (((size_t)j * S + row) << log2d) + n, count = n_slabs;
    else if (row == S) dst = ga + ((size_t)j << log2d) + n, count = S * n_slabs;
    else p += 2 * D, dst = gc + ((size_t)j << log2d) + n, count = S * n_slabs;
    float acc = 0.0f;
    uint32_t k = 0;
    for (; k + 8 <= count; k += 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[(size_t)(k + i) * ps];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = acc + v[i];
    }
    for (; k < count; ++k) acc = acc + p[(size_t)k * ps];
    *dst = acc;
}

// Every argument check of whvi_fused_shs_stacked_bwd_f32, before any device call (fused_bwd_check's order).  WHVI_OK with
// launch = false: nothing to launch.
static int fused_stacked_bwd_check(FusedStackedBwdArgs &r, bool &launch, void *grad_x, void *grad_a, void *grad_b, void *grad_c,
                                   void *work, const void *grad_y, const void *x, const void *a, const void *b, const void *c,
                                   int64_t J, int64_t S, int64_t stride, int32_t log2d, int32_t flags)
{
    g_err[0] = 0;
    launch = false;
    if (flags & ~WHVI_FUSED_SRC_SHARED)
        return fail(WHVI_ERR_ARG, "whvi_fused_shs_stacked_bwd: unknown fused flags%s 0x%llx (0 or the shared-source flag)", "", flags);
    if (J < 0 || S < 0 || stride < 0) return fail(WHVI_ERR_ARG, "whvi_fused_shs_stacked_bwd: negative size%s", "");
    if (!fused_stacked_bwd_supported(log2d, J))
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_bwd: %s%lld blocks of log2(D) = %lld are outside the supported range "
                    "(2 .. 4 blocks for 6 <= log2(D) <= 10, 2 blocks at 11)", "", J, log2d);
    if (S == 0 || stride == 0) return WHVI_OK;
    if (!grad_a || !grad_b || !grad_c || !work || !grad_y || !x || !a || !b || !c)
        return fail(WHVI_ERR_ARG, "whvi_fused_shs_stacked_bwd: null pointer%s (only grad_x may be NULL)", "");
    if (S >= ((int64_t)1 << 32) / stride)
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_bwd: rows are indexed with 32 bits%s", "");
    if ((J * (S + 2) << log2d) >= ((int64_t)1 << 31))
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_bwd: gradients are indexed with 32 bits%s", "");
    if (((uintptr_t)grad_x | (uintptr_t)grad_a | (uintptr_t)grad_b | (uintptr_t)grad_c | (uintptr_t)work | (uintptr_t)grad_y |
         (uintptr_t)x | (uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15)
        return fail(WHVI_ERR_ALIGN, "whvi_fused_shs_stacked_bwd: a pointer%s is not 16-byte aligned", "");
    const FusedBwdGeom geom = fused_bwd_geom(S, stride, log2d);
    if (S * geom.n_slabs >= ((int64_t)1 << 31)) return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_bwd: too many blocks%s", "");
    const int64_t row_bytes = (int64_t)4 << log2d, rows = S * stride;
    const bool shared = (flags & WHVI_FUSED_SRC_SHARED) != 0;
    const struct { const void *p; int64_t bytes; } outs[] = {
        {grad_x, rows * row_bytes}, {grad_a, J * row_bytes}, {grad_b, J * S * row_bytes}, {grad_c, J * row_bytes},
        {work, S * geom.n_slabs * fused_stacked_bwd_part_floats(log2d, J) * 4}};
    const struct { const void *p; int64_t bytes; } ins[] = {
        {grad_y, rows * J * row_bytes}, {x, (shared ? stride : rows) * row_bytes}, {a, J * row_bytes}, {b, J * S * row_bytes},
        {c, J * row_bytes}};
    for (const auto &o : outs) {
        if (o.p == nullptr) continue;
        for (const auto &t : ins)
            if (ranges_overlap(o.p, o.bytes, t.p, t.bytes))
                return fail(WHVI_ERR_OVERLAP, "whvi_fused_shs_stacked_bwd: grad_x, a parameter gradient or the workspace overlaps "
                            "an input%s", "");
    }
    r.grad_x = grad_x, r.work = work, r.grad_y = grad_y, r.x = x, r.a = a, r.b = b, r.c = c;
    r.n_blocks = J, r.n_samples = S, r.sample_stride = stride, r.log2d = log2d, r.x_shared = shared, r.geom = geom;
    // the streamed bytes: the J segments of grad_y, x unless shared, grad_x unless skipped
    r.nt = rows * row_bytes * (J + (shared ? 0 : 1) + (grad_x != nullptr ? 1 : 0)) > NT_MIN_BYTES;
    launch = true;
    return WHVI_OK;
}

template <int L>
static void fused_stacked_bwd_launch(const FusedStackedBwdArgs &r, hipStream_t st)
{
    if constexpr (L <= 10) {
        switch (r.n_blocks) {
        case 2: fused_stacked_bwd_launch_one<float, L, 2>(r, st); break;
        case 3: fused_stacked_bwd_launch_one<float, L, 3>(r, st); break;
        default: fused_stacked_bwd_launch_one<float, L, 4>(r, st); break;
        }
    } else {
        fused_stacked_bwd_launch_one<float, L, 2>(r, st);
    }
}

}  // namespace whvi

using namespace whvi;

WHVI_EXPORT int whvi_fused_shs_stacked_bwd_supported(int32_t log2d, int64_t n_blocks)
{
    return fused_stacked_bwd_supported(log2d, n_blocks) ? 1 : 0;
}

WHVI_EXPORT int64_t whvi_fused_shs_stacked_bwd_workspace(int64_t n_samples, int64_t sample_stride, int32_t log2d, int64_t n_blocks)
{
    if (n_samples < 0 || sample_stride < 0 || n_blocks < 0) return WHVI_ERR_ARG;
    if (!fused_stacked_bwd_supported(log2d, n_blocks)) return WHVI_ERR_SIZE;
    if (n_samples == 0 || sample_stride == 0) return 0;
    return n_samples * fused_bwd_geom(n_samples, sample_stride, log2d).n_slabs * fused_stacked_bwd_part_floats(log2d, n_blocks) *
           (int64_t)sizeof(float);
}

WHVI_EXPORT int whvi_fused_shs_stacked_bwd_f32(void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *work,
                                               const void *grad_y, const void *x, const void *a, const void *b, const void *c,
                                               int64_t n_blocks, int64_t n_samples, int64_t sample_stride, int32_t log2d,
                                               int32_t flags, void *stream)
{
    FusedStackedBwdArgs r;
    bool launch = false;
    int rc = fused_stacked_bwd_check(r, launch, grad_x, grad_a, grad_b, grad_c, work, grad_y, x, a, b, c, n_blocks, n_samples,
                                     sample_stride, log2d, flags);
    if (rc != WHVI_OK || !launch) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (log2d) {
    case 6: fused_stacked_bwd_launch<6>(r, st); break;
    case 7: fused_stacked_bwd_launch<7>(r, st); break;
    case 8: fused_stacked_bwd_launch<8>(r, st); break;
    case 9: fused_stacked_bwd_launch<9>(r, st); break;
    case 10: fused_stacked_bwd_launch<10>(r, st); break;
    default: fused_stacked_bwd_launch<11>(r, st); break;
    }
    rc = after_launch("fused_shs_stacked_bwd");
    if (rc != WHVI_OK) return rc;
    const int64_t total = n_blocks * (n_samples + 2) << log2d;
    hipLaunchKernelGGL(fused_shs_stacked_bwd_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (float *)grad_a,
                       (float *)grad_b, (float *)grad_c, (const float *)r.work, (uint32_t)n_blocks, (uint32_t)n_samples,
                       (uint32_t)r.geom.n_slabs, (uint32_t)log2d);
    return after_launch("fused_shs_stacked_bwd (finish)");
}
