// whvi_amd/csrc/mlp_apply.hip -- the predictive pass of a WHVI regression network (first layer, 1 .. 4 square layers, row
// dot) for all Monte-Carlo samples in one launch, f32.  ABI: include/whvi_hip.h (whvi_mlp_apply_f32, whvi_mlp_apply_supported).
#include "dispatch.hpp"
#include "mlp_apply.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

namespace whvi {

static int mlp_apply_dispatch(void *y, const void *x, int32_t first, const void *w_in, const void *b_in, int32_t n_mid,
                              const void *s1, const void *s2, const void *u, const void *b_mid, int32_t mid_bias,
                              const void *w_out, const void *b_out, int64_t S, int64_t B, int32_t log2d, int32_t relu,
                              void *stream)
{
    g_err[0] = 0;
    MlpLaunch ln;
    const int rc = mlp_apply_check(ln, y, x, first, w_in, b_in, n_mid, s1, s2, u, b_mid, mid_bias, w_out, b_out, S, B, log2d, relu,
                                   "relu");
    if (rc != WHVI_OK || ln.grid.x == 0) return rc;
    const dim3 grid = ln.grid;
    const size_t lds = ln.lds;
    const uint32_t slab_rows = ln.slab_rows, n_slabs = ln.n_slabs;
    hipStream_t st = (hipStream_t)stream;
#define WHVI_MLP(L, K)                                                                                          \
    do {                                                                                                        \
        if constexpr (mlp_lds_bytes(K, 1, L) <= MLP_MAX_LDS) {                                                  \
            note_launch<float>("mlp_apply_kernel", L, K);                                                       \
            hipLaunchKernelGGL((mlp_apply_kernel<float, L, K>), grid, dim3(256), lds, st, (float *)y, (const float *)x, \
                               (const float *)w_in, (const float *)b_in, (const float *)s1, (const float *)s2,   \
                               (const float *)u, (const float *)b_mid, (const float *)w_out, (const float *)b_out, \
                               (uint32_t)S, (uint32_t)B, (uint32_t)n_mid, (uint32_t)mid_bias, (uint32_t)relu,    \
                               slab_rows, n_slabs);                                                             \
        }                                                                                                       \
    } while (0)
#define WHVI_CASE(L)                                                                                            \
    case L:                                                                                                     \
        if (first == 1) WHVI_MLP(L, 1); else if (first == 4) WHVI_MLP(L, 4); else WHVI_MLP(L, 8);               \
        break;
    switch (log2d) {
        WHVI_CASE(6) WHVI_CASE(7) WHVI_CASE(8) WHVI_CASE(9) WHVI_CASE(10) WHVI_CASE(11)
    default: break;
    }
#undef WHVI_CASE
#undef WHVI_MLP
    return after_launch("mlp_apply");
}

}  // namespace whvi

WHVI_EXPORT int whvi_mlp_apply_supported(int32_t first, int32_t n_mid, int32_t log2d)
{
    return whvi::mlp_supported(first, n_mid, log2d) ? 1 : 0;
}

WHVI_EXPORT int whvi_mlp_apply_f32(void *y, const void *x, int32_t first, const void *w_in, const void *b_in, int32_t n_mid,
                                   const void *s1, const void *s2, const void *u, const void *b_mid, int32_t mid_bias,
                                   const void *w_out, const void *b_out, int64_t S, int64_t B, int32_t log2d, int32_t relu,
                                   void *stream)
{
    return whvi::mlp_apply_dispatch(y, x, first, w_in, b_in, n_mid, s1, s2, u, b_mid, mid_bias, w_out, b_out, S, B, log2d, relu,
                                    stream);
}
