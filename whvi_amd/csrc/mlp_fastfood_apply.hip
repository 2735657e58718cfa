// whvi_amd/csrc/mlp_fastfood_apply.hip -- the one-launch predictive pass of a WHVI regression network whose square layers are
// fastfood layers (whvi_amd/fastfood.py), f32.  ABI: include/whvi_hip.h (whvi_mlp_fastfood_apply_f32,
// whvi_mlp_fastfood_apply_supported).
//
//     WHVILinear(n_in, D) [act] WHVILinear(D, D, mode="fastfood") [act] ... [act] WHVILinear(D, 1)
//
// The geometry, the first layer, the activations and the output layer are mlp_apply.hpp's (same helpers, same lane layout);
// each square layer is the batched route's fused_shs_kernel (kernels.hpp) followed by its torch bias add, per row:
//     t = s2 * h;  FWHT;  t = g_k * t;  FWHT;  h = s1 * t;  (+ bias, its own rounding);  (activation)
// A lane's R x C chunks of the hidden vector are exactly fwht_tile's tile layout -- index k 256 + lane 4 + c with k = r C + j:
// rows of D >= 256 own the six lane bits and C k-bits, shorter rows leave the upper lane bits and every k-bit to the row
// index, which fwht_tile never butterflies.  Both transforms are fwht_tile with the fused kernel's template arguments (the
// signed DPP network, stages in ascending stride), so every butterfly rounds -- and every zero gets its sign -- as there:
// the result is bit-identical to fused_shs + torch add + activation.  There is no row-poison rule in these layers (the
// batched route has none): non-finite values propagate through the butterflies.
//
// LDS per block: that sample's W1 ([c][n]), b_in, w_out and per square layer s2, g_k, s1, bias -- 4 D (K + 2 + 4 n_mid) bytes,
// at most 64 KiB.  No atomics, no scratch.
#include "mlp_fastfood_apply.hpp"

#define WHVI_EXPORT extern "C" __attribute__((visibility("default")))

namespace whvi {

// y[s, b] for b in the block's slab.  x : (B, KIN); w_in : (S, D, KIN) (KIN = 4 / 8) or (S, D) (KIN = 1); s1, s2, b_mid :
// (n_mid, D); g : (n_mid, S, D); w_out : (S, D).  act bit 0: the activation behind the first layer, bit 1 + m: behind
// square layer m.  mid_bias bit m: square layer m has a bias.  ACT: WHVI_MLP_ACT_*.
template <typename T, int LOG2D, int KIN, int ACT>      // (T = float; named so that whvi_last_kernel prints the real symbol)
__global__ void __launch_bounds__(256)
mlp_fastfood_apply_kernel(float *__restrict__ y, const float *__restrict__ x, const float *__restrict__ w_in,
                          const float *__restrict__ b_in, const float *__restrict__ s1, const float *__restrict__ s2,
                          const float *__restrict__ g, const float *__restrict__ b_mid, const float *__restrict__ w_out,
                          const float *__restrict__ b_out, uint32_t S, uint32_t B, uint32_t n_mid, uint32_t mid_bias,
                          uint32_t act, uint32_t slab_rows, uint32_t n_slabs)
{
    using Gm = MlpGeom<LOG2D>;
    using Act = typename MlpAct<ACT>::type;
    constexpr int D = Gm::D, L = Gm::L, C = Gm::C, R = Gm::R, RPI = Gm::RPI;
    typedef float f4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float mlp_lds[];
    float *lw1 = mlp_lds;                    // [c][n]: KIN rows of D
    float *lbi = lw1 + KIN * D;              // b_in
    float *lwo = lbi + D;                    // w_out
    float *lff = lwo + D;                    // square layer m at 4 m D: s2, g_k, s1, bias

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t b0 = slab * slab_rows, b1 = b0 + slab_rows < B ? b0 + slab_rows : B;

    mlp_ff_stage_operands<LOG2D, KIN>(mlp_lds, s, w_in, b_in, s1, s2, g, b_mid, w_out, S, n_mid, mid_bias);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t grp = (uint32_t)lane / L, col = (uint32_t)lane % L;      // the lane's row group and first chunk
    const bool has_b_in = b_in != nullptr;
    const float bo = b_out != nullptr ? b_out[0] : 0.0f;
    float *ys = y + (size_t)s * B;
    // the loop bound is wave-uniform (rows past b1 compute on a valid row's operands and are never stored): every lane of
    // the wave takes part in the DPP / permlane stages of the transforms
    for (uint32_t rb = b0 + wave * RPI; rb < b1; rb += 4 * RPI) {
        // D >= 1024: re-read the operands from LDS on every iteration rather than hoisting them into registers (mlp_apply.hpp)
        if constexpr (C >= 4) asm volatile("" ::: "memory");
        const uint32_t r0 = rb + grp * R;
        float h[R][C][4];
        {   // ---- first layer
            float xv[R][KIN];
            mlp_load_x<KIN, R>(xv, x, r0, b1);
            mlp_first_layer<LOG2D, KIN, R, Act>(h, xv, lw1, lbi, col, has_b_in, (act & 1u) != 0);
        }
        // ---- fastfood square layers
        for (uint32_t m = 0; m < n_mid; ++m)
            mlp_ff_layer<LOG2D, R, Act>(h, lff + 4 * m * D, lane, col, (mid_bias >> m) & 1u, (act >> (m + 1)) & 1u);
        // ---- transposed column layer: row_dot_kernel's partials, order and butterfly (as mlp_apply_kernel)
        float acc[R];
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const f4 wc = reinterpret_cast<const f4 *>(lwo)[col + j * L];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float a = h[r][j][0] * wc[0];
#pragma unroll
                for (int e = 1; e < 4; ++e) a = __builtin_fmaf(h[r][j][e], wc[e], a);
                acc[r] = j == 0 ? a : acc[r] + a;
            }
        }
        float outv = 0.0f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float v = acc[r];
#pragma unroll
            for (int m = 1; m < L; m <<= 1) v = v + __shfl_xor(v, m, 64);
            if (col == (uint32_t)r) outv = v;
        }
        if (b_out != nullptr) outv = outv + bo;
        if (col < (uint32_t)R && r0 + col < b1) ys[r0 + col] = outv;
    }
}

// Every argument check of whvi_mlp_fastfood_apply_f32, before any launch.  WHVI_OK with ln.grid.x = 0: nothing to launch.
static int mlp_ff_check(MlpLaunch &ln, const void *y, const void *x, int32_t first, const void *w_in, const void *b_in,
                        int32_t n_mid, const void *s1, const void *s2, const void *g, const void *b_mid, int32_t mid_bias,
                        const void *w_out, const void *b_out, int64_t S, int64_t B, int32_t log2d, int32_t act, int32_t act_bits)
{
    ln.grid = dim3(0);
    if (act != WHVI_MLP_ACT_RELU && act != WHVI_MLP_ACT_SIGMOID && act != WHVI_MLP_ACT_TANH)
        return fail(WHVI_ERR_ARG, "whvi_mlp_fastfood_apply: unknown act%s %lld (1 relu, 2 sigmoid, 3 tanh)", "", act);
    if (S < 0 || B < 0) return fail(WHVI_ERR_ARG, "whvi_mlp_fastfood_apply: negative size%s", "");
    if (first != WHVI_MLP_FIRST_COLUMN && first != WHVI_MLP_FIRST_K4 && first != WHVI_MLP_FIRST_K8)
        return fail(WHVI_ERR_ARG, "whvi_mlp_fastfood_apply: unknown first-layer kind%s %lld", "", first);
    if (n_mid < 1 || n_mid > MLP_MAX_MID)
        return fail(WHVI_ERR_SIZE, "whvi_mlp_fastfood_apply: n_mid%s = %lld square layers (1 .. 4 only)", "", n_mid);
    if (log2d < 6 || log2d > 11)
        return fail(WHVI_ERR_SIZE, "whvi_mlp_fastfood_apply: log2(D)%s = %lld is outside [6, 11]", "", log2d);
    if (!mlp_ff_supported(first, n_mid, log2d))
        return fail(WHVI_ERR_SIZE, "whvi_mlp_fastfood_apply: the operands of one sample%s need %lld B of LDS (64 KiB at most)", "",
                    mlp_ff_lds_bytes(first, n_mid, log2d));
    if (act_bits & ~((1 << (n_mid + 1)) - 1))
        return fail(WHVI_ERR_ARG, "whvi_mlp_fastfood_apply: unknown act_bits%s 0x%llx", "", act_bits);
    if (mid_bias & ~((1 << n_mid) - 1))
        return fail(WHVI_ERR_ARG, "whvi_mlp_fastfood_apply: unknown mid_bias bits%s 0x%llx", "", mid_bias);
    const int64_t rows = S * B;
    if (rows == 0) return WHVI_OK;
    if (rows >= ((int64_t)1 << 32)) return fail(WHVI_ERR_SIZE, "whvi_mlp_fastfood_apply: rows are indexed with 32 bits%s", "");
    if (!y || !x || !w_in || !s1 || !s2 || !g || !w_out || (mid_bias != 0 && !b_mid))
        return fail(WHVI_ERR_ARG, "whvi_mlp_fastfood_apply: null pointer%s", "");
    if (((uintptr_t)y | (uintptr_t)x | (uintptr_t)w_in | (uintptr_t)b_in | (uintptr_t)s1 | (uintptr_t)s2 | (uintptr_t)g |
         (uintptr_t)b_mid | (uintptr_t)w_out | (uintptr_t)b_out) & 15)
        return fail(WHVI_ERR_ALIGN, "whvi_mlp_fastfood_apply: a pointer%s is not 16-byte aligned", "");
    {
        const int64_t D = (int64_t)1 << log2d, kin = first;
        const struct { const void *p; int64_t n; } in[] = {
            {x, B * kin}, {w_in, S * D * kin}, {b_in, D}, {s1, n_mid * D}, {s2, n_mid * D}, {g, n_mid * S * D},
            {b_mid, n_mid * D}, {w_out, S * D}, {b_out, 1}};
        const char *yp = (const char *)y, *ye = yp + rows * 4;
        for (const auto &t : in) {
            const char *p = (const char *)t.p;
            if (p != nullptr && p < ye && yp < p + t.n * 4)
                return fail(WHVI_ERR_OVERLAP, "whvi_mlp_fastfood_apply: y overlaps an input%s", "");
        }
    }
    // slabs: mlp_apply_check's rule -- about four blocks per CU over all samples, every wave with at least one row group
    int64_t n_slabs = (4 * (int64_t)num_cu() + S - 1) / S;
    const int64_t min_rows = 4 * 64;
    const int64_t most = (B + min_rows - 1) / min_rows;
    if (n_slabs > most) n_slabs = most;
    if (n_slabs < 1) n_slabs = 1;
    const int64_t slab_rows = (B + n_slabs - 1) / n_slabs;
    n_slabs = (B + slab_rows - 1) / slab_rows;
    if (n_slabs * S >= ((int64_t)1 << 31)) return fail(WHVI_ERR_SIZE, "whvi_mlp_fastfood_apply: too many blocks%s", "");
    ln.lds = (size_t)mlp_ff_lds_bytes(first, n_mid, log2d);
    ln.grid = dim3((unsigned)(n_slabs * S));
    ln.slab_rows = (uint32_t)slab_rows;
    ln.n_slabs = (uint32_t)n_slabs;
    return WHVI_OK;
}

static int mlp_ff_dispatch(void *y, const void *x, int32_t first, const void *w_in, const void *b_in, int32_t n_mid,
                           const void *s1, const void *s2, const void *g, const void *b_mid, int32_t mid_bias, const void *w_out,
                           const void *b_out, int64_t S, int64_t B, int32_t log2d, int32_t act, int32_t act_bits, void *stream)
{
    g_err[0] = 0;
    MlpLaunch ln;
    const int rc = mlp_ff_check(ln, y, x, first, w_in, b_in, n_mid, s1, s2, g, b_mid, mid_bias, w_out, b_out, S, B, log2d, act,
                                act_bits);
    if (rc != WHVI_OK || ln.grid.x == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
#define WHVI_MLPF(L, K, A)                                                                                      \
    do {                                                                                                        \
        if constexpr (mlp_ff_lds_bytes(K, 1, L) <= MLP_MAX_LDS) {                                               \
            note_launch<float>("mlp_fastfood_apply_kernel", L, K, A);                                           \
            hipLaunchKernelGGL((mlp_fastfood_apply_kernel<float, L, K, A>), ln.grid, dim3(256), ln.lds, st, (float *)y, \
                               (const float *)x, (const float *)w_in, (const float *)b_in, (const float *)s1,   \
                               (const float *)s2, (const float *)g, (const float *)b_mid, (const float *)w_out, \
                               (const float *)b_out, (uint32_t)S, (uint32_t)B, (uint32_t)n_mid, (uint32_t)mid_bias, \
                               (uint32_t)act_bits, ln.slab_rows, ln.n_slabs);                                   \
        }                                                                                                       \
    } while (0)
#define WHVI_MLPF_K(L, K)                                                                                       \
    if (act == WHVI_MLP_ACT_RELU) WHVI_MLPF(L, K, WHVI_MLP_ACT_RELU);                                           \
    else if (act == WHVI_MLP_ACT_SIGMOID) WHVI_MLPF(L, K, WHVI_MLP_ACT_SIGMOID);                                \
    else WHVI_MLPF(L, K, WHVI_MLP_ACT_TANH);
#define WHVI_CASE(L)                                                                                            \
    case L:                                                                                                     \
        if (first == 1) { WHVI_MLPF_K(L, 1) } else if (first == 4) { WHVI_MLPF_K(L, 4) } else { WHVI_MLPF_K(L, 8) } \
        break;
    switch (log2d) {
        WHVI_CASE(6) WHVI_CASE(7) WHVI_CASE(8) WHVI_CASE(9) WHVI_CASE(10) WHVI_CASE(11)
    default: break;
    }
#undef WHVI_CASE
#undef WHVI_MLPF_K
#undef WHVI_MLPF
    return after_launch("mlp_fastfood_apply");
}

}  // namespace whvi

WHVI_EXPORT int whvi_mlp_fastfood_apply_supported(int32_t first, int32_t n_mid, int32_t log2d)
{
    return whvi::mlp_ff_supported(first, n_mid, log2d) ? 1 : 0;
}

WHVI_EXPORT int whvi_mlp_fastfood_apply_f32(void *y, const void *x, int32_t first, const void *w_in, const void *b_in,
                                            int32_t n_mid, const void *s1, const void *s2, const void *g, const void *b_mid,
                                            int32_t mid_bias, const void *w_out, const void *b_out, int64_t S, int64_t B,
                                            int32_t log2d, int32_t act, int32_t act_bits, void *stream)
{
    return whvi::mlp_ff_dispatch(y, x, first, w_in, b_in, n_mid, s1, s2, g, b_mid, mid_bias, w_out, b_out, S, B, log2d, act,
                                 act_bits, stream);
}
