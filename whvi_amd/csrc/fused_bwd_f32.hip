// whvi_amd/csrc/fused_bwd_f32.hip -- one-launch backward of the fused scale/FWHT/scale/FWHT/scale pipeline, float: the
// instantiations of fused_shs_bwd_kernel (fused_bwd.hpp), the finishing launch and the ABI (include/whvi_hip.h:
// whvi_fused_shs_bwd_supported, whvi_fused_shs_bwd_workspace, whvi_fused_shs_bwd_f32), and the argument checks and the
// finishing launch that the 16-bit entries (fused_bwd_f16.hip, fused_bwd_bf16.hip) share.  Built like fused_f32.hip:
// -ffp-contract=off -fno-slp-vectorize.
#include "dispatch.hpp"
#include "fused_bwd.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

namespace whvi {

// Slots in ascending block order.  Thread t < S D: grad_b[s][n] over the n_slabs blocks of sample s; the next D threads:
// grad_a[n] over all S n_slabs blocks; the last D: grad_c[n].  Eight loads in flight, added in order.
__global__ void __launch_bounds__(256)
fused_shs_bwd_finish_kernel(float *__restrict__ ga, float *__restrict__ gb, float *__restrict__ gc,
                            const float *__restrict__ part, uint32_t S, uint32_t n_slabs, uint32_t log2d)
{
    const uint32_t D = 1u << log2d;
    const size_t ps = (size_t)3 << log2d;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= (S + 2) * D) return;
    const uint32_t n = t & (D - 1), row = t >> log2d;
    const float *p;
    float *dst;
    uint32_t count;
    if (row < S) p = part + (size_t)row * n_slabs * ps + D + n, dst = gb + ((size_t)row << log2d) + n, count = n_slabs;
    else if (row == S) p = part + n, dst = ga + n, count = S * n_slabs;
    else p = part + 2 * D + n, dst = gc + n, count = S * n_slabs;
    float acc = 0.0f;
    uint32_t k = 0;
    for (; k + 8 <= count; k += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(k + j) * ps];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = acc + v[j];
    }
    for (; k < count; ++k) acc = acc + p[(size_t)k * ps];
    *dst = acc;
}

// Every argument check of whvi_fused_shs_bwd_f32 / _f16 / _bf16 (act_bytes = 4 / 2 / 2: the element of x, grad_y and grad_x),
// before any device call.  WHVI_OK with launch = false: nothing to launch.
int fused_bwd_check(FusedBwdArgs &r, bool &launch, void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *work,
                    const void *grad_y, const void *x, const void *a, const void *b, const void *c, int64_t S, int64_t stride,
                    int32_t log2d, int32_t flags, int64_t act_bytes)
{
    g_err[0] = 0;
    launch = false;
    if (flags & ~WHVI_FUSED_SRC_SHARED)
        return fail(WHVI_ERR_ARG, "whvi_fused_shs_bwd: unknown fused flags%s 0x%llx (0 or the shared-source flag)", "", flags);
    if (S < 0 || stride < 0) return fail(WHVI_ERR_ARG, "whvi_fused_shs_bwd: negative size%s", "");
    if (!fused_bwd_supported(log2d))
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_bwd: log2(D)%s = %lld is outside the supported range [6, %lld]", "", log2d,
                    FUSED_BWD_MAX_LOG2D);
    if (S == 0 || stride == 0) return WHVI_OK;
    if (!grad_a || !grad_b || !grad_c || !work || !grad_y || !x || !a || !b || !c)
        return fail(WHVI_ERR_ARG, "whvi_fused_shs_bwd: null pointer%s (only grad_x may be NULL)", "");
    if (S >= ((int64_t)1 << 32) / stride)
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_bwd: rows are indexed with 32 bits%s", "");
    if (((S + 2) << log2d) >= ((int64_t)1 << 31))
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_bwd: gradients are indexed with 32 bits%s", "");
    if (((uintptr_t)grad_x | (uintptr_t)grad_a | (uintptr_t)grad_b | (uintptr_t)grad_c | (uintptr_t)work | (uintptr_t)grad_y |
         (uintptr_t)x | (uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15)
        return fail(WHVI_ERR_ALIGN, "whvi_fused_shs_bwd: a pointer%s is not 16-byte aligned", "");
    const FusedBwdGeom geom = fused_bwd_geom(S, stride, log2d);
    if (S * geom.n_slabs >= ((int64_t)1 << 31)) return fail(WHVI_ERR_SIZE, "whvi_fused_shs_bwd: too many blocks%s", "");
    const int64_t D = (int64_t)1 << log2d, rows = S * stride;
    const bool shared = (flags & WHVI_FUSED_SRC_SHARED) != 0;
    const struct { const void *p; int64_t bytes; } outs[] = {
        {grad_x, rows * D * act_bytes}, {grad_a, D * 4}, {grad_b, S * D * 4}, {grad_c, D * 4},
        {work, S * geom.n_slabs * fused_bwd_part_floats(log2d) * 4}};
    const struct { const void *p; int64_t bytes; } ins[] = {
        {grad_y, rows * D * act_bytes}, {x, (shared ? stride : rows) * D * act_bytes}, {a, D * 4}, {b, S * D * 4}, {c, D * 4}};
    for (const auto &o : outs) {
        if (o.p == nullptr) continue;
        for (const auto &t : ins)
            if (ranges_overlap(o.p, o.bytes, t.p, t.bytes))
                return fail(WHVI_ERR_OVERLAP, "whvi_fused_shs_bwd: grad_x, a parameter gradient or the workspace overlaps an "
                            "input%s", "");
    }
    r.grad_x = grad_x, r.work = work, r.grad_y = grad_y, r.x = x, r.a = a, r.b = b, r.c = c;
    r.n_samples = S, r.sample_stride = stride, r.log2d = log2d, r.x_shared = shared, r.geom = geom;
    // the streamed bytes: grad_y, x unless shared, grad_x unless skipped
    r.nt = rows * D * act_bytes * (1 + (shared ? 0 : 1) + (grad_x != nullptr ? 1 : 0)) > NT_MIN_BYTES;
    launch = true;
    return WHVI_OK;
}

int fused_bwd_finish(const FusedBwdArgs &r, void *grad_a, void *grad_b, void *grad_c, hipStream_t st)
{
    const int64_t total = (r.n_samples + 2) << r.log2d;
    hipLaunchKernelGGL(fused_shs_bwd_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (float *)grad_a,
                       (float *)grad_b, (float *)grad_c, (const float *)r.work, (uint32_t)r.n_samples, (uint32_t)r.geom.n_slabs,
                       (uint32_t)r.log2d);
    return after_launch("fused_shs_bwd (finish)");
}

}  // namespace whvi

using namespace whvi;

WHVI_EXPORT int whvi_fused_shs_bwd_supported(int32_t log2d) { return fused_bwd_supported(log2d) ? 1 : 0; }

WHVI_EXPORT int64_t whvi_fused_shs_bwd_workspace(int64_t n_samples, int64_t sample_stride, int32_t log2d)
{
    if (n_samples < 0 || sample_stride < 0) return WHVI_ERR_ARG;
    if (!fused_bwd_supported(log2d)) return WHVI_ERR_SIZE;
    if (n_samples == 0 || sample_stride == 0) return 0;
    return n_samples * fused_bwd_geom(n_samples, sample_stride, log2d).n_slabs * fused_bwd_part_floats(log2d) * (int64_t)sizeof(float);
}

WHVI_EXPORT int whvi_fused_shs_bwd_f32(void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *work, const void *grad_y,
                                       const void *x, const void *a, const void *b, const void *c, int64_t n_samples,
                                       int64_t sample_stride, int32_t log2d, int32_t flags, void *stream)
{
    return fused_bwd_run<float>(grad_x, grad_a, grad_b, grad_c, work, grad_y, x, a, b, c, n_samples, sample_stride, log2d, flags,
                                stream);
}
