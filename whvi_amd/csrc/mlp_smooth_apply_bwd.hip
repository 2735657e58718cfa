// whvi_amd/csrc/mlp_smooth_apply_bwd.hip -- backward of whvi_mlp_apply_act_f32, f32.  ABI: include/whvi_hip.h
// (whvi_mlp_apply_act_bwd_f32).  ReLU networks run whvi_mlp_apply_bwd_f32's kernels (mlp_apply_bwd.hip); the smooth
// activations' backward kernels are instantiated here and share its finishing launch.
#include "dispatch.hpp"
#include "mlp_apply_bwd.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

namespace whvi {

// whvi_mlp_apply_act_bwd_f32 with a smooth activation (act = WHVI_MLP_ACT_SIGMOID / _TANH; the caller checked act)
static int mlp_smooth_apply_bwd_dispatch(void *grad_w_in, void *grad_w_mid, void *grad_w_out, void *grad_b, void *grad_x,
                                         void *work, int64_t work_floats, const void *g, const void *x, int32_t first,
                                         const void *w_in, const void *b_in, int32_t n_mid, const void *s1, const void *s2,
                                         const void *u, const void *b_mid, int32_t mid_bias, const void *w_out, int64_t S,
                                         int64_t B, int32_t log2d, int32_t act, int32_t act_bits, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MlpBwdLaunch ln;
    int rc = mlp_apply_bwd_check(ln, grad_w_in, grad_w_mid, grad_w_out, grad_b, grad_x, work, work_floats, g, x, first, w_in, b_in,
                                 n_mid, s1, s2, u, b_mid, mid_bias, w_out, S, B, log2d, act_bits, "act", st);
    if (rc != WHVI_OK || ln.grid.x == 0) return rc;
#define WHVI_MLPSB(L, K, N, A)                                                                                  \
    do {                                                                                                        \
        if constexpr (mlp_lds_bytes(K, N, L) <= MLP_MAX_LDS) {                                                  \
            note_launch<float>("mlp_smooth_apply_bwd_kernel", L, K, N, A);                                      \
            hipLaunchKernelGGL((mlp_smooth_apply_bwd_kernel<float, L, K, N, A>), ln.grid, dim3(256), ln.lds, st, \
                               (float *)work, (float *)grad_x, (const float *)g, (const float *)x, (const float *)w_in, \
                               (const float *)b_in, (const float *)s1, (const float *)s2, (const float *)u,     \
                               (const float *)b_mid, (const float *)w_out, (uint32_t)S, (uint32_t)B,            \
                               (uint32_t)mid_bias, (uint32_t)act_bits, ln.slab_rows, ln.n_slabs);               \
        }                                                                                                       \
    } while (0)
#define WHVI_MLPSB_N(L, K, N)                                                                                   \
    if (act == WHVI_MLP_ACT_SIGMOID) WHVI_MLPSB(L, K, N, WHVI_MLP_ACT_SIGMOID); else WHVI_MLPSB(L, K, N, WHVI_MLP_ACT_TANH);
#define WHVI_MLPSB_K(L, K)                                                                                      \
    if (n_mid == 1) { WHVI_MLPSB_N(L, K, 1) } else { WHVI_MLPSB_N(L, K, 2) }
#define WHVI_CASE(L)                                                                                            \
    case L:                                                                                                     \
        if (first == 1) { WHVI_MLPSB_K(L, 1) } else if (first == 4) { WHVI_MLPSB_K(L, 4) } else { WHVI_MLPSB_K(L, 8) } \
        break;
    switch (log2d) {
        WHVI_CASE(6) WHVI_CASE(7) WHVI_CASE(8) WHVI_CASE(9) WHVI_CASE(10)
    default: break;
    }
#undef WHVI_CASE
#undef WHVI_MLPSB_K
#undef WHVI_MLPSB_N
#undef WHVI_MLPSB
    rc = after_launch("mlp_apply_bwd");
    if (rc != WHVI_OK) return rc;
    return mlp_apply_bwd_finish(grad_w_in, grad_w_mid, grad_w_out, grad_b, work, S, ln.n_slabs, first, n_mid, log2d, st);
}

}  // namespace whvi

WHVI_EXPORT int whvi_mlp_apply_act_bwd_f32(void *grad_w_in, void *grad_w_mid, void *grad_w_out, void *grad_b, void *grad_x,
                                           void *work, int64_t work_floats, const void *g, const void *x, int32_t first,
                                           const void *w_in, const void *b_in, int32_t n_mid, const void *s1, const void *s2,
                                           const void *u, const void *b_mid, int32_t mid_bias, const void *w_out, int64_t S,
                                           int64_t B, int32_t log2d, int32_t act, int32_t act_bits, void *stream)
{
    whvi::g_err[0] = 0;
    if (act == WHVI_MLP_ACT_RELU)
        return whvi_mlp_apply_bwd_f32(grad_w_in, grad_w_mid, grad_w_out, grad_b, grad_x, work, work_floats, g, x, first, w_in, b_in,
                                      n_mid, s1, s2, u, b_mid, mid_bias, w_out, S, B, log2d, act_bits, stream);
    if (act != WHVI_MLP_ACT_SIGMOID && act != WHVI_MLP_ACT_TANH)
        return whvi::fail(WHVI_ERR_ARG, "whvi_mlp_apply_bwd: unknown act%s %lld (1 relu, 2 sigmoid, 3 tanh)", "", act);
    return whvi::mlp_smooth_apply_bwd_dispatch(grad_w_in, grad_w_mid, grad_w_out, grad_b, grad_x, work, work_floats, g, x, first,
                                               w_in, b_in, n_mid, s1, s2, u, b_mid, mid_bias, w_out, S, B, log2d, act, act_bits,
                                               stream);
}
