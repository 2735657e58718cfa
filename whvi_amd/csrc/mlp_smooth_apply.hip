// whvi_amd/csrc/mlp_smooth_apply.hip -- the one-launch predictive pass of a WHVI regression network with a choice of
// activation, f32.  ABI: include/whvi_hip.h (whvi_mlp_apply_act_f32).  ReLU networks run whvi_mlp_apply_f32's kernels
// (mlp_apply.hip); the smooth activations (sigmoid, tanh) are instantiated here.
#include "dispatch.hpp"
#include "mlp_apply.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

namespace whvi {

// whvi_mlp_apply_act_f32 with a smooth activation (act = WHVI_MLP_ACT_SIGMOID / _TANH; the caller checked act)
static int mlp_smooth_apply_dispatch(void *y, const void *x, int32_t first, const void *w_in, const void *b_in, int32_t n_mid,
                                     const void *s1, const void *s2, const void *u, const void *b_mid, int32_t mid_bias,
                                     const void *w_out, const void *b_out, int64_t S, int64_t B, int32_t log2d, int32_t act,
                                     int32_t act_bits, void *stream)
{
    MlpLaunch ln;
    const int rc = mlp_apply_check(ln, y, x, first, w_in, b_in, n_mid, s1, s2, u, b_mid, mid_bias, w_out, b_out, S, B, log2d,
                                   act_bits, "act");
    if (rc != WHVI_OK || ln.grid.x == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
#define WHVI_MLPS(L, K, A)                                                                                      \
    do {                                                                                                        \
        if constexpr (mlp_lds_bytes(K, 1, L) <= MLP_MAX_LDS) {                                                  \
            note_launch<float>("mlp_smooth_apply_kernel", L, K, A);                                             \
            hipLaunchKernelGGL((mlp_smooth_apply_kernel<float, L, K, A>), ln.grid, dim3(256), ln.lds, st, (float *)y, \
                               (const float *)x, (const float *)w_in, (const float *)b_in, (const float *)s1,   \
                               (const float *)s2, (const float *)u, (const float *)b_mid, (const float *)w_out, \
                               (const float *)b_out, (uint32_t)S, (uint32_t)B, (uint32_t)n_mid, (uint32_t)mid_bias, \
                               (uint32_t)act_bits, ln.slab_rows, ln.n_slabs);                                   \
        }                                                                                                       \
    } while (0)
#define WHVI_MLPS_K(L, K)                                                                                       \
    if (act == WHVI_MLP_ACT_SIGMOID) WHVI_MLPS(L, K, WHVI_MLP_ACT_SIGMOID); else WHVI_MLPS(L, K, WHVI_MLP_ACT_TANH);
#define WHVI_CASE(L)                                                                                            \
    case L:                                                                                                     \
        if (first == 1) { WHVI_MLPS_K(L, 1) } else if (first == 4) { WHVI_MLPS_K(L, 4) } else { WHVI_MLPS_K(L, 8) } \
        break;
    switch (log2d) {
        WHVI_CASE(6) WHVI_CASE(7) WHVI_CASE(8) WHVI_CASE(9) WHVI_CASE(10) WHVI_CASE(11)
    default: break;
    }
#undef WHVI_CASE
#undef WHVI_MLPS_K
#undef WHVI_MLPS
    return after_launch("mlp_apply");
}

}  // namespace whvi

WHVI_EXPORT int whvi_mlp_apply_act_f32(void *y, const void *x, int32_t first, const void *w_in, const void *b_in, int32_t n_mid,
                                       const void *s1, const void *s2, const void *u, const void *b_mid, int32_t mid_bias,
                                       const void *w_out, const void *b_out, int64_t S, int64_t B, int32_t log2d, int32_t act,
                                       int32_t act_bits, void *stream)
{
    whvi::g_err[0] = 0;
    if (act == WHVI_MLP_ACT_RELU)
        return whvi_mlp_apply_f32(y, x, first, w_in, b_in, n_mid, s1, s2, u, b_mid, mid_bias, w_out, b_out, S, B, log2d, act_bits,
                                  stream);
    if (act != WHVI_MLP_ACT_SIGMOID && act != WHVI_MLP_ACT_TANH)
        return whvi::fail(WHVI_ERR_ARG, "whvi_mlp_apply: unknown act%s %lld (1 relu, 2 sigmoid, 3 tanh)", "", act);
    return whvi::mlp_smooth_apply_dispatch(y, x, first, w_in, b_in, n_mid, s1, s2, u, b_mid, mid_bias, w_out, b_out, S, B, log2d,
                                           act, act_bits, stream);
}
