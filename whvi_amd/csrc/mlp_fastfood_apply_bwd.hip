// whvi_amd/csrc/mlp_fastfood_apply_bwd.hip -- backward of the one-launch pass of a WHVI regression network with fastfood square
// layers, f32: the ReLU instantiations, the finishing launch and the ABI (include/whvi_hip.h: whvi_mlp_fastfood_apply_bwd_f32,
// whvi_mlp_fastfood_apply_bwd_supported, whvi_mlp_fastfood_apply_bwd_workspace).  The sigmoid and tanh instantiations are
// compiled in mlp_fastfood_smooth_apply_bwd.hip.
#include "dispatch.hpp"
#include "mlp_fastfood_apply_bwd.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

namespace whvi {

WHVI_MLP_FF_BWD_DEFINE(mlp_ff_bwd_launch_relu, WHVI_MLP_ACT_RELU)

// Slabs in ascending order.  Thread t < S (K + n_mid + 1) D: one per-sample output, (field, s, n) with n fastest -- grad_w_in's
// K columns, grad_g's n_mid layers, grad_w_out; then (1 + 3 n_mid) D + 1 sums over samples and slabs: b_in, the n_mid biases,
// the n_mid grad_s1, the n_mid grad_s2, b_out.
__global__ void __launch_bounds__(256)
mlp_fastfood_apply_bwd_finish_kernel(float *__restrict__ gw_in, float *__restrict__ gs1, float *__restrict__ gs2,
                                     float *__restrict__ gg, float *__restrict__ gw_out, float *__restrict__ gb,
                                     const float *__restrict__ part, uint32_t S, uint32_t n_slabs, uint32_t kin, uint32_t n_mid,
                                     uint32_t log2d)
{
    const uint32_t D = 1u << log2d, F = kin + 2 + 4 * n_mid;
    const size_t ps = ((size_t)F << log2d) + 4;
    const uint32_t n_per = S * (kin + n_mid + 1) * D, n_sum = (1 + 3 * n_mid) * D + 1;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_per + n_sum) return;
    if (t < n_per) {
        const uint32_t n = t & (D - 1), fs = t >> log2d, s = fs % S, fi = fs / S;
        const uint32_t field = fi < kin ? fi : (fi < kin + n_mid ? kin + 1 + 4 * (fi - kin) + 1 : F - 1);
        const float *p = part + (size_t)s * n_slabs * ps + (size_t)field * D + n;
        float a = 0.0f;
        for (uint32_t k = 0; k < n_slabs; ++k) a = a + p[(size_t)k * ps];
        if (fi < kin) gw_in[((size_t)s * D + n) * kin + fi] = a;
        else if (fi < kin + n_mid) gg[((size_t)(fi - kin) * S + s) * D + n] = a;
        else gw_out[(size_t)s * D + n] = a;
        return;
    }
    const uint32_t tb = t - n_per, fb = tb >> log2d, n = tb & (D - 1);
    size_t off;
    float *dst;
    if (fb == 0) {
        off = (size_t)kin * D + n, dst = gb + n;                                               // b_in
    } else if (fb <= n_mid) {
        off = (size_t)(kin + 1 + 4 * (fb - 1) + 3) * D + n, dst = gb + (size_t)fb * D + n;      // square layer fb - 1's bias
    } else if (fb <= 2 * n_mid) {
        off = (size_t)(kin + 1 + 4 * (fb - 1 - n_mid) + 2) * D + n, dst = gs1 + (size_t)(fb - 1 - n_mid) * D + n;
    } else if (fb <= 3 * n_mid) {
        off = (size_t)(kin + 1 + 4 * (fb - 1 - 2 * n_mid)) * D + n, dst = gs2 + (size_t)(fb - 1 - 2 * n_mid) * D + n;
    } else {
        off = (size_t)F * D, dst = gb + (size_t)(1 + n_mid) * D;                               // b_out: sum g
    }
    float a = 0.0f;
    for (size_t k = 0; k < (size_t)S * n_slabs; ++k) a = a + part[k * ps + off];
    *dst = a;
}

// Every argument check of whvi_mlp_fastfood_apply_bwd_f32, before any launch.  B = 0 zero-fills the gradients here.  WHVI_OK
// with ln.grid.x = 0: nothing to launch.
static int mlp_ff_bwd_check(MlpBwdLaunch &ln, void *grad_w_in, void *grad_s1, void *grad_s2, void *grad_g, void *grad_w_out,
                            void *grad_b, void *grad_x, void *work, int64_t work_floats, const void *g, const void *x,
                            int32_t first, const void *w_in, const void *b_in, int32_t n_mid, const void *s1, const void *s2,
                            const void *gk, const void *b_mid, int32_t mid_bias, const void *w_out, int64_t S, int64_t B,
                            int32_t log2d, int32_t act, int32_t act_bits, hipStream_t st)
{
    ln.grid = dim3(0);
    if (act != WHVI_MLP_ACT_RELU && act != WHVI_MLP_ACT_SIGMOID && act != WHVI_MLP_ACT_TANH)
        return fail(WHVI_ERR_ARG, "whvi_mlp_fastfood_apply_bwd: unknown act%s %lld (1 relu, 2 sigmoid, 3 tanh)", "", act);
    if (S < 0 || B < 0) return fail(WHVI_ERR_ARG, "whvi_mlp_fastfood_apply_bwd: negative size%s", "");
    if (first != WHVI_MLP_FIRST_COLUMN && first != WHVI_MLP_FIRST_K4 && first != WHVI_MLP_FIRST_K8)
        return fail(WHVI_ERR_ARG, "whvi_mlp_fastfood_apply_bwd: unknown first-layer kind%s %lld", "", first);
    if (!mlp_ff_bwd_supported(first, n_mid, log2d))
        return fail(WHVI_ERR_SIZE, "whvi_mlp_fastfood_apply_bwd: unsupported network%s (n_mid = %lld, log2(D) = %lld; see "
                    "whvi_mlp_fastfood_apply_bwd_supported)", "", n_mid, log2d);
    if (act_bits & ~((1 << (n_mid + 1)) - 1))
        return fail(WHVI_ERR_ARG, "whvi_mlp_fastfood_apply_bwd: unknown act_bits%s 0x%llx", "", act_bits);
    if (mid_bias & ~((1 << n_mid) - 1))
        return fail(WHVI_ERR_ARG, "whvi_mlp_fastfood_apply_bwd: unknown mid_bias bits%s 0x%llx", "", mid_bias);
    if (S == 0) return WHVI_OK;
    if (S * B >= ((int64_t)1 << 32)) return fail(WHVI_ERR_SIZE, "whvi_mlp_fastfood_apply_bwd: rows are indexed with 32 bits%s", "");
    if (((S * (first + n_mid + 1) + 1 + 3 * n_mid) << log2d) >= ((int64_t)1 << 31))
        return fail(WHVI_ERR_SIZE, "whvi_mlp_fastfood_apply_bwd: gradients are indexed with 32 bits%s", "");
    if (!grad_w_in || !grad_s1 || !grad_s2 || !grad_g || !grad_w_out || !grad_b || !w_in || !s1 || !s2 || !gk || !w_out ||
        (mid_bias != 0 && !b_mid) || (B > 0 && (!work || !g || !x)))
        return fail(WHVI_ERR_ARG, "whvi_mlp_fastfood_apply_bwd: null pointer%s", "");
    if (((uintptr_t)grad_w_in | (uintptr_t)grad_s1 | (uintptr_t)grad_s2 | (uintptr_t)grad_g | (uintptr_t)grad_w_out |
         (uintptr_t)grad_b | (uintptr_t)grad_x | (uintptr_t)work | (uintptr_t)g | (uintptr_t)x | (uintptr_t)w_in | (uintptr_t)b_in |
         (uintptr_t)s1 | (uintptr_t)s2 | (uintptr_t)gk | (uintptr_t)b_mid | (uintptr_t)w_out) & 15)
        return fail(WHVI_ERR_ALIGN, "whvi_mlp_fastfood_apply_bwd: a pointer%s is not 16-byte aligned", "");
    const int64_t n_slabs = mlp_bwd_slabs(S, B);
    const int64_t need = B > 0 ? S * n_slabs * mlp_ff_bwd_part_floats(first, n_mid, log2d) : 0;
    if (work_floats < need)
        return fail(WHVI_ERR_ARG, "whvi_mlp_fastfood_apply_bwd: workspace of%s %lld floats, %lld needed "
                    "(whvi_mlp_fastfood_apply_bwd_workspace)", "", work_floats, need);
    const int64_t D = (int64_t)1 << log2d, kin = first;
    const struct { const void *p; int64_t n; } outs[] = {
        {grad_w_in, S * D * kin}, {grad_s1, n_mid * D}, {grad_s2, n_mid * D}, {grad_g, n_mid * S * D}, {grad_w_out, S * D},
        {grad_b, (1 + n_mid) * D + 1}, {grad_x, S * B * kin}, {work, need}};
    const struct { const void *p; int64_t n; } ins[] = {
        {g, S * B}, {x, B * kin}, {w_in, S * D * kin}, {b_in, D}, {s1, n_mid * D}, {s2, n_mid * D}, {gk, n_mid * S * D},
        {b_mid, n_mid * D}, {w_out, S * D}};
    for (const auto &o : outs) {
        const char *op = (const char *)o.p, *oe = op + o.n * 4;
        if (op == nullptr || o.n == 0) continue;
        for (const auto &t : ins) {
            const char *p = (const char *)t.p;
            if (p != nullptr && t.n > 0 && p < oe && op < p + t.n * 4)
                return fail(WHVI_ERR_OVERLAP, "whvi_mlp_fastfood_apply_bwd: an output or the workspace overlaps an input%s", "");
        }
    }
    if (B == 0) {                                          // no rows: every gradient is an empty sum
        for (int i = 0; i < 6; ++i)
            if (hipMemsetAsync((void *)outs[i].p, 0, (size_t)outs[i].n * 4, st) != hipSuccess)
                return fail(WHVI_ERR_LAUNCH, "whvi_mlp_fastfood_apply_bwd: memset%s", "");
        return WHVI_OK;
    }
    const int64_t slab_rows = (B + n_slabs - 1) / n_slabs;
    if (n_slabs * S >= ((int64_t)1 << 31)) return fail(WHVI_ERR_SIZE, "whvi_mlp_fastfood_apply_bwd: too many blocks%s", "");
    ln.lds = (size_t)mlp_ff_lds_bytes(first, n_mid, log2d) + 16;
    ln.grid = dim3((unsigned)(n_slabs * S));
    ln.slab_rows = (uint32_t)slab_rows;
    ln.n_slabs = (uint32_t)n_slabs;
    return WHVI_OK;
}

static int mlp_ff_bwd_dispatch(void *grad_w_in, void *grad_s1, void *grad_s2, void *grad_g, void *grad_w_out, void *grad_b,
                               void *grad_x, void *work, int64_t work_floats, const void *g, const void *x, int32_t first,
                               const void *w_in, const void *b_in, int32_t n_mid, const void *s1, const void *s2, const void *gk,
                               const void *b_mid, int32_t mid_bias, const void *w_out, int64_t S, int64_t B, int32_t log2d,
                               int32_t act, int32_t act_bits, void *stream)
{
    g_err[0] = 0;
    hipStream_t st = (hipStream_t)stream;
    MlpFfBwdArgs a;
    int rc = mlp_ff_bwd_check(a.ln, grad_w_in, grad_s1, grad_s2, grad_g, grad_w_out, grad_b, grad_x, work, work_floats, g, x, first,
                              w_in, b_in, n_mid, s1, s2, gk, b_mid, mid_bias, w_out, S, B, log2d, act, act_bits, st);
    if (rc != WHVI_OK || a.ln.grid.x == 0) return rc;
    a.grad_x = grad_x, a.work = work, a.g = g, a.x = x, a.w_in = w_in, a.b_in = b_in, a.s1 = s1, a.s2 = s2, a.gk = gk;
    a.b_mid = b_mid, a.w_out = w_out, a.first = first, a.n_mid = n_mid, a.mid_bias = mid_bias, a.log2d = log2d;
    a.act_bits = act_bits, a.S = S, a.B = B;
    if (act == WHVI_MLP_ACT_RELU) mlp_ff_bwd_launch_relu(a, st);
    else if (act == WHVI_MLP_ACT_SIGMOID) mlp_ff_bwd_launch_sigmoid(a, st);
    else mlp_ff_bwd_launch_tanh(a, st);
    rc = after_launch("mlp_fastfood_apply_bwd");
    if (rc != WHVI_OK) return rc;
    const int64_t D = (int64_t)1 << log2d;
    const int64_t total = S * (first + n_mid + 1) * D + (1 + 3 * n_mid) * D + 1;
    hipLaunchKernelGGL(mlp_fastfood_apply_bwd_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       (float *)grad_w_in, (float *)grad_s1, (float *)grad_s2, (float *)grad_g, (float *)grad_w_out,
                       (float *)grad_b, (const float *)work, (uint32_t)S, a.ln.n_slabs, (uint32_t)first, (uint32_t)n_mid,
                       (uint32_t)log2d);
    return after_launch("mlp_fastfood_apply_bwd (finish)");
}

}  // namespace whvi

WHVI_EXPORT int whvi_mlp_fastfood_apply_bwd_supported(int32_t first, int32_t n_mid, int32_t log2d)
{
    return whvi::mlp_ff_bwd_supported(first, n_mid, log2d) ? 1 : 0;
}

WHVI_EXPORT int64_t whvi_mlp_fastfood_apply_bwd_workspace(int64_t S, int64_t B, int32_t first, int32_t n_mid, int32_t log2d)
{
    if (S < 0 || B < 0 || !whvi::mlp_ff_bwd_supported(first, n_mid, log2d)) return -1;
    if (S == 0 || B == 0) return 0;
    return S * whvi::mlp_bwd_slabs(S, B) * whvi::mlp_ff_bwd_part_floats(first, n_mid, log2d);
}

WHVI_EXPORT int whvi_mlp_fastfood_apply_bwd_f32(void *grad_w_in, void *grad_s1, void *grad_s2, void *grad_g, void *grad_w_out,
                                                void *grad_b, void *grad_x, void *work, int64_t work_floats, const void *g,
                                                const void *x, int32_t first, const void *w_in, const void *b_in, int32_t n_mid,
                                                const void *s1, const void *s2, const void *gk, const void *b_mid,
                                                int32_t mid_bias, const void *w_out, int64_t S, int64_t B, int32_t log2d,
                                                int32_t act, int32_t act_bits, void *stream)
{
    return whvi::mlp_ff_bwd_dispatch(grad_w_in, grad_s1, grad_s2, grad_g, grad_w_out, grad_b, grad_x, work, work_floats, g, x,
                                     first, w_in, b_in, n_mid, s1, s2, gk, b_mid, mid_bias, w_out, S, B, log2d, act, act_bits,
                                     stream);
}
