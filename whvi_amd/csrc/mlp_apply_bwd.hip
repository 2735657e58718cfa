// whvi_amd/csrc/mlp_apply_bwd.hip -- backward of the one-launch predictive pass of a WHVI regression network, f32.
// ABI: include/whvi_hip.h (whvi_mlp_apply_bwd_f32, whvi_mlp_apply_bwd_supported, whvi_mlp_apply_bwd_workspace).
#include "dispatch.hpp"
#include "mlp_apply_bwd.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

namespace whvi {

// Slabs in ascending order.  Thread t < S (K + n_mid + 1) D: one per-sample output, (field, s, n) with n fastest; then
// (1 + n_mid) D + 1 bias sums over samples and slabs.
__global__ void __launch_bounds__(256)
mlp_apply_bwd_finish_kernel(float *__restrict__ gw_in, float *__restrict__ gw_mid, float *__restrict__ gw_out,
                            float *__restrict__ gb, const float *__restrict__ part, uint32_t S, uint32_t n_slabs, uint32_t kin,
                            uint32_t n_mid, uint32_t log2d)
{
    const uint32_t D = 1u << log2d, F = kin + 2 + 2 * n_mid;
    const size_t ps = ((size_t)F << log2d) + 4;
    const uint32_t n_per = S * (kin + n_mid + 1) * D, n_bias = (1 + n_mid) * D + 1;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_per + n_bias) return;
    if (t < n_per) {
        const uint32_t n = t & (D - 1), fs = t >> log2d, s = fs % S, fi = fs / S;
        const uint32_t field = fi < kin ? fi : (fi < kin + n_mid ? fi + 1 : F - 1);
        const float *p = part + (size_t)s * n_slabs * ps + (size_t)field * D + n;
        float a = 0.0f;
        for (uint32_t k = 0; k < n_slabs; ++k) a = a + p[(size_t)k * ps];
        if (fi < kin) gw_in[((size_t)s * D + n) * kin + fi] = a;
        else if (fi < kin + n_mid) gw_mid[((size_t)(fi - kin) * S + s) * D + n] = a;
        else gw_out[(size_t)s * D + n] = a;
        return;
    }
    const uint32_t tb = t - n_per;
    size_t off;
    if (tb < (1 + n_mid) * D) {
        const uint32_t fb = tb >> log2d, n = tb & (D - 1);
        off = (size_t)(fb == 0 ? kin : kin + 1 + n_mid + (fb - 1)) * D + n;
    } else {
        off = (size_t)F * D;
    }
    float a = 0.0f;
    for (size_t k = 0; k < (size_t)S * n_slabs; ++k) a = a + part[k * ps + off];
    gb[tb] = a;
}

int mlp_apply_bwd_finish(void *grad_w_in, void *grad_w_mid, void *grad_w_out, void *grad_b, const void *work, int64_t S,
                         int64_t n_slabs, int32_t first, int32_t n_mid, int32_t log2d, hipStream_t st)
{
    const int64_t D = (int64_t)1 << log2d;
    const int64_t total = S * (first + n_mid + 1) * D + (1 + n_mid) * D + 1;
    hipLaunchKernelGGL(mlp_apply_bwd_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (float *)grad_w_in,
                       (float *)grad_w_mid, (float *)grad_w_out, (float *)grad_b, (const float *)work, (uint32_t)S,
                       (uint32_t)n_slabs, (uint32_t)first, (uint32_t)n_mid, (uint32_t)log2d);
    return after_launch("mlp_apply_bwd (finish)");
}

static int mlp_apply_bwd_dispatch(void *grad_w_in, void *grad_w_mid, void *grad_w_out, void *grad_b, void *grad_x, void *work,
                                  int64_t work_floats, const void *g, const void *x, int32_t first, const void *w_in,
                                  const void *b_in, int32_t n_mid, const void *s1, const void *s2, const void *u,
                                  const void *b_mid, int32_t mid_bias, const void *w_out, int64_t S, int64_t B, int32_t log2d,
                                  int32_t relu, void *stream)
{
    g_err[0] = 0;
    hipStream_t st = (hipStream_t)stream;
    MlpBwdLaunch ln;
    int rc = mlp_apply_bwd_check(ln, grad_w_in, grad_w_mid, grad_w_out, grad_b, grad_x, work, work_floats, g, x, first, w_in, b_in,
                                 n_mid, s1, s2, u, b_mid, mid_bias, w_out, S, B, log2d, relu, "relu", st);
    if (rc != WHVI_OK || ln.grid.x == 0) return rc;
    const dim3 grid = ln.grid;
    const size_t lds = ln.lds;
#define WHVI_MLPB(L, K, N)                                                                                      \
    do {                                                                                                        \
        if constexpr (mlp_lds_bytes(K, N, L) <= MLP_MAX_LDS) {                                                  \
            note_launch<float>("mlp_apply_bwd_kernel", L, K, N);                                                \
            hipLaunchKernelGGL((mlp_apply_bwd_kernel<float, L, K, N>), grid, dim3(256), lds, st, (float *)work,   \
                               (float *)grad_x, (const float *)g, (const float *)x, (const float *)w_in,        \
                               (const float *)b_in, (const float *)s1, (const float *)s2, (const float *)u,     \
                               (const float *)b_mid, (const float *)w_out, (uint32_t)S, (uint32_t)B,            \
                               (uint32_t)mid_bias, (uint32_t)relu, ln.slab_rows, ln.n_slabs);                   \
        }                                                                                                       \
    } while (0)
#define WHVI_MLPB_K(L, K)                                                                                       \
    if (n_mid == 1) WHVI_MLPB(L, K, 1); else WHVI_MLPB(L, K, 2);
#define WHVI_CASE(L)                                                                                            \
    case L:                                                                                                     \
        if (first == 1) { WHVI_MLPB_K(L, 1) } else if (first == 4) { WHVI_MLPB_K(L, 4) } else { WHVI_MLPB_K(L, 8) } \
        break;
    switch (log2d) {
        WHVI_CASE(6) WHVI_CASE(7) WHVI_CASE(8) WHVI_CASE(9) WHVI_CASE(10)
    default: break;
    }
#undef WHVI_CASE
#undef WHVI_MLPB_K
#undef WHVI_MLPB
    rc = after_launch("mlp_apply_bwd");
    if (rc != WHVI_OK) return rc;
    return mlp_apply_bwd_finish(grad_w_in, grad_w_mid, grad_w_out, grad_b, work, S, ln.n_slabs, first, n_mid, log2d, st);
}

}  // namespace whvi

WHVI_EXPORT int whvi_mlp_apply_bwd_supported(int32_t first, int32_t n_mid, int32_t log2d)
{
    return whvi::mlp_bwd_supported(first, n_mid, log2d) ? 1 : 0;
}

WHVI_EXPORT int64_t whvi_mlp_apply_bwd_workspace(int64_t S, int64_t B, int32_t first, int32_t n_mid, int32_t log2d)
{
    return whvi::mlp_apply_bwd_workspace(S, B, first, n_mid, log2d);
}

WHVI_EXPORT int whvi_mlp_apply_bwd_f32(void *grad_w_in, void *grad_w_mid, void *grad_w_out, void *grad_b, void *grad_x,
                                       void *work, int64_t work_floats, const void *g, const void *x, int32_t first,
                                       const void *w_in, const void *b_in, int32_t n_mid, const void *s1, const void *s2,
                                       const void *u, const void *b_mid, int32_t mid_bias, const void *w_out, int64_t S,
                                       int64_t B, int32_t log2d, int32_t relu, void *stream)
{
    return whvi::mlp_apply_bwd_dispatch(grad_w_in, grad_w_mid, grad_w_out, grad_b, grad_x, work, work_floats, g, x, first, w_in,
                                        b_in, n_mid, s1, s2, u, b_mid, mid_bias, w_out, S, B, log2d, relu, stream);
}
