// whvi_amd/csrc/fused_stacked_layer_bwd_f16.hip -- one-launch backward of the rectangular fastfood layer with its epilogue (the
// masks of both ReLUs, the zero padding past n_cols and the bias sum folded in), __half activations with float32 scale vectors,
// gradients and workspace: the instantiations of fused_layer_bwd16_kernel<__half, ...> (fused_stacked_layer_bwd16.hpp; one
// translation unit per dtype so the library builds in parallel), and -- once for both dtypes -- the argument checks, the
// finishing launch and the support query.  ABI: include/whvi_hip.h (whvi_fused_shs_stacked_layer_bwd16_supported,
// whvi_fused_shs_stacked_layer_bwd_f16).  Built like fused_stacked_bwd_f16.hip: -ffp-contract=off -fno-slp-vectorize.
#include "dispatch.hpp"
#include "fused_stacked_layer_bwd16.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

namespace whvi {

constexpr int32_t FUSED_LAYER_BWD16_FLAGS = WHVI_FUSED_SRC_SHARED | WHVI_FUSED_RELU_IN | WHVI_FUSED_RELU_OUT;

// Slots of [j][a | b | c][D] (then [j][bias][D] with R = 3) in ascending block order, added as the float32 launch's finishing
// kernel adds them.  Per j, (S + R) D threads: thread t < S D: grad_b[j][s][n] over the n_slabs blocks of sample s; the next
// D: grad_a[j][n] over all S n_slabs blocks; the next D: grad_c[j][n]; with a bias the last D: grad_bias[j D + n], +0 from
// n_cols on.  Eight loads in flight, added in order.
__global__ void __launch_bounds__(256)
fused_layer_bwd16_finish_kernel(float *__restrict__ ga, float *__restrict__ gb, float *__restrict__ gc, float *__restrict__ gbias,
                                const float *__restrict__ part, uint32_t J, uint32_t S, uint32_t n_slabs, uint32_t log2d,
                                uint32_t n_cols)
{
    const uint32_t D = 1u << log2d, R = gbias != nullptr ? 3u : 2u;
    const size_t ps = (size_t)(R + 1) * J << log2d;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= J * (S + R) * D) return;
    const uint32_t n = t & (D - 1), jrow = t >> log2d, j = jrow / (S + R), row = jrow - j * (S + R);
    const float *p = part + ((size_t)3 * j << log2d) + n;
    float *dst;
    uint32_t count;
    if (row < S) p += (size_t)row * n_slabs * ps + D, dst = gb + (((size_t)j * S + row) << log2d) + n, count = n_slabs;
    else if (row == S) dst = ga + ((size_t)j << log2d) + n, count = S * n_slabs;
    else if (row == S + 1) p += 2 * D, dst = gc + ((size_t)j << log2d) + n, count = S * n_slabs;
    else {
        p = part + ((size_t)(3 * J + j) << log2d) + n, dst = gbias + ((size_t)j << log2d) + n, count = S * n_slabs;
        if ((j << log2d) + n >= n_cols) {
            *dst = 0.0f;
            return;
        }
    }
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

int fused_layer_bwd16_check(FusedStackedLayerBwdArgs &r, bool &launch, void *grad_x, void *grad_a, void *grad_b, void *grad_c,
                            void *grad_bias, void *work, const void *grad_y, const void *y, const void *x, const void *a,
                            const void *b, const void *c, int64_t J, int64_t S, int64_t stride, int32_t log2d, int64_t n_cols,
                            int64_t ld, int32_t flags)
{
    g_err[0] = 0;
    launch = false;
    if (flags & ~FUSED_LAYER_BWD16_FLAGS)
        return fail(WHVI_ERR_ARG, "whvi_fused_shs_stacked_layer_bwd16: unknown fused flags%s 0x%llx (shared source, ReLU in, ReLU out)",
                    "", flags);
    if (J < 0 || S < 0 || stride < 0 || n_cols < 0 || ld < 0)
        return fail(WHVI_ERR_ARG, "whvi_fused_shs_stacked_layer_bwd16: negative size%s", "");
    const bool bias = grad_bias != nullptr, relu_out = (flags & WHVI_FUSED_RELU_OUT) != 0;
    if (!fused_layer_bwd16_supported(log2d, J, bias))
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer_bwd16: %s%lld blocks of log2(D) = %lld are outside the supported "
                    "range (2 .. 4 blocks for 6 <= log2(D) <= 10, 2 blocks at 11)", "", J, log2d);
    if ((n_cols | ld) & 7)
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer_bwd16: n_cols%s = %lld and ld = %lld must be multiples of 8", "",
                    n_cols, ld);
    if (n_cols <= ((J - 1) << log2d) || n_cols > (J << log2d))
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer_bwd16: n_cols%s = %lld must end in the last of the %lld blocks", "",
                    n_cols, J);
    if (ld < n_cols || ld >= ((int64_t)1 << 32))
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer_bwd16: ld%s = %lld is below n_cols = %lld (or beyond 32 bits)", "", ld,
                    n_cols);
    if (S == 0 || stride == 0) return WHVI_OK;
    if (!grad_a || !grad_b || !grad_c || !work || !grad_y || !x || !a || !b || !c)
        return fail(WHVI_ERR_ARG, "whvi_fused_shs_stacked_layer_bwd16: null pointer%s (only grad_x and grad_bias may be NULL)", "");
    if (relu_out != (y != nullptr))
        return fail(WHVI_ERR_ARG, "whvi_fused_shs_stacked_layer_bwd16: y%s is given exactly with the ReLU-out flag", "");
    if (S >= ((int64_t)1 << 32) / stride)
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer_bwd16: rows are indexed with 32 bits%s", "");
    if (S * stride > (((int64_t)1 << 60) / ld))          // (rows, ld < 2^32: the spans of grad_y and y below stay inside 64 bits)
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer_bwd16: rows * ld%s is beyond 2^60 elements", "");
    if ((J * (S + (bias ? 3 : 2)) << log2d) >= ((int64_t)1 << 31))
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer_bwd16: gradients are indexed with 32 bits%s", "");
    if (((uintptr_t)grad_x | (uintptr_t)grad_a | (uintptr_t)grad_b | (uintptr_t)grad_c | (uintptr_t)grad_bias | (uintptr_t)work |
         (uintptr_t)grad_y | (uintptr_t)y | (uintptr_t)x | (uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15)
        return fail(WHVI_ERR_ALIGN, "whvi_fused_shs_stacked_layer_bwd16: a pointer%s is not 16-byte aligned", "");
    const FusedBwdGeom geom = fused_bwd_geom(S, stride, log2d);
    if (S * geom.n_slabs >= ((int64_t)1 << 31))
        return fail(WHVI_ERR_SIZE, "whvi_fused_shs_stacked_layer_bwd16: too many blocks%s", "");
    // a row of x / grad_x in bytes (2-byte activations), and a float32 vector
    const int64_t act_row = (int64_t)2 << log2d, vec_bytes = (int64_t)4 << log2d, rows = S * stride;
    const bool shared = (flags & WHVI_FUSED_SRC_SHARED) != 0;
    const struct { const void *p; int64_t bytes; } outs[] = {
        {grad_x, rows * act_row}, {grad_a, J * vec_bytes}, {grad_b, J * S * vec_bytes}, {grad_c, J * vec_bytes},
        {grad_bias, J * vec_bytes}, {work, S * geom.n_slabs * fused_stacked_layer_bwd_part_floats(log2d, J, bias) * 4}};
    const struct { const void *p; int64_t bytes; } ins[] = {
        {grad_y, rows * ld * 2}, {y, rows * ld * 2}, {x, (shared ? stride : rows) * act_row}, {a, J * vec_bytes},
        {b, J * S * vec_bytes}, {c, J * vec_bytes}};
    for (const auto &o : outs) {
        if (o.p == nullptr) continue;
        for (const auto &t : ins)
            if (t.p != nullptr && ranges_overlap(o.p, o.bytes, t.p, t.bytes))
                return fail(WHVI_ERR_OVERLAP, "whvi_fused_shs_stacked_layer_bwd16: grad_x, a parameter gradient or the workspace "
                            "overlaps an input%s", "");
    }
    r.grad_x = grad_x, r.grad_bias = grad_bias, r.work = work, r.grad_y = grad_y, r.y = y, r.x = x, r.a = a, r.b = b, r.c = c;
    r.n_blocks = J, r.n_samples = S, r.sample_stride = stride, r.n_cols = n_cols, r.ld = ld, r.log2d = log2d;
    r.opts = ((flags & WHVI_FUSED_RELU_IN) ? LAYER_BWD_OPT_RELU_IN : 0u) | (relu_out ? LAYER_BWD_OPT_RELU_OUT : 0u);
    r.x_shared = shared, r.geom = geom;
    // the streamed bytes: the n_cols columns of grad_y (and of y), x unless shared, grad_x unless skipped
    r.nt = rows * 2 * (n_cols * (relu_out ? 2 : 1) + ((int64_t)(shared ? 0 : 1) << log2d) + ((int64_t)(grad_x != nullptr ? 1 : 0) << log2d)) >
           NT_MIN_BYTES;
    launch = true;
    return WHVI_OK;
}

int fused_layer_bwd16_finish(const FusedStackedLayerBwdArgs &r, void *grad_a, void *grad_b, void *grad_c, hipStream_t st)
{
    const int64_t total = r.n_blocks * (r.n_samples + (r.grad_bias != nullptr ? 3 : 2)) << r.log2d;
    hipLaunchKernelGGL(fused_layer_bwd16_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (float *)grad_a,
                       (float *)grad_b, (float *)grad_c, (float *)r.grad_bias, (const float *)r.work, (uint32_t)r.n_blocks,
                       (uint32_t)r.n_samples, (uint32_t)r.geom.n_slabs, (uint32_t)r.log2d, (uint32_t)r.n_cols);
    return after_launch("fused_shs_stacked_layer_bwd (16-bit, finish)");
}

}  // namespace whvi

using namespace whvi;

WHVI_EXPORT int whvi_fused_shs_stacked_layer_bwd16_supported(int32_t log2d, int64_t n_blocks, int32_t has_bias)
{
    return fused_layer_bwd16_supported(log2d, n_blocks, has_bias != 0) ? 1 : 0;
}

WHVI_EXPORT int whvi_fused_shs_stacked_layer_bwd_f16(void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *grad_bias,
                                                     void *work, const void *grad_y, const void *y, const void *x, const void *a,
                                                     const void *b, const void *c, int64_t n_blocks, int64_t n_samples,
                                                     int64_t sample_stride, int32_t log2d, int64_t n_cols, int64_t ld,
                                                     int32_t flags, void *stream)
{
    return fused_layer_bwd16_run<__half>(grad_x, grad_a, grad_b, grad_c, grad_bias, work, grad_y, y, x, a, b, c, n_blocks,
                                         n_samples, sample_stride, log2d, n_cols, ld, flags, stream);
}
