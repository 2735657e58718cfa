#pragma once
// whvi_amd/csrc/mlp_apply_bwd.hpp -- backward of whvi_mlp_apply_f32 (mlp_apply.hpp): the parameter gradients of a WHVI regression
// network of the canonical shape for ALL Monte-Carlo samples from g = dL/dy, without any saved activation.
//
// A block owns (sample s, a slab of batch rows), stages the sample's operands in LDS exactly as the forward does and recomputes
// each row's hidden vectors with the forward's helpers (mlp_first_layer, mlp_square_layer: same arithmetic, so the same ReLU
// masks and the same poisoned rows as the three-launch route).  It then runs that route's backward formulas element by element:
//   output layer (RowDotFunction)      d = g * w_out;  grad_w_out += h_L * g
//   square layer m (whvi_diag_apply_bwd) d = 0 where its fused ReLU's recomputed pre-activation (from the layer's input before
//                                      the poison) has relu_(z) <= 0;  grad_w_mid[m] += d * h_{m-1};  grad_b_mid[m] += d;
//                                      d = d * w_m
//   first layer                         ReLU behind it: column layer (the square layer's relu_in) d = 0 where h_0 <= 0; stacked
//                                      layer (SmallKApplyFunction) d = d * (h_0 > 0);  grad_b_in += d;
//                                      grad_w_in[n, c] += d * x[c];  grad_x[s, b, c] = sum_n d * w_in[n, c] (a butterfly)
// With a smooth activation (mlp_smooth_apply_bwd_kernel, ACT = WHVI_MLP_ACT_SIGMOID / _TANH) the two activation steps above are
// torch's formula on the recomputed output y (hs[]): sigmoid d = (d * (1 - y)) * y, tanh d = d * (1 - y * y) -- no masks.
// Each lane keeps the sums of its hidden units over its rows in registers (C * 4 * (K + 2 + 2 n_mid) floats); lane groups of a
// wave combine by a butterfly, the four waves through LDS in wave order, and the block writes one partial per field to its slab
// of the workspace.  A second, tiny launch inside the same call adds the slabs in ascending order (samples in ascending order
// for the bias sums): deterministic, no atomics, no allocation.
#include "mlp_apply.hpp"

namespace whvi {

constexpr int MLP_BWD_MAX_MID = 2;
constexpr int MLP_BWD_MAX_LOG2D = 10;

template <int LOG2D> struct MlpBwdGeom {
    using Gm = MlpGeom<LOG2D>;
    static constexpr int R = Gm::C >= 4 ? 1 : 4 / Gm::C;  // R x C = 4 chunks: 16 hidden floats per lane and layer
    static constexpr int RPI = Gm::G * R;                 // rows per wave iteration
};

// partial sums per block: fields [0, K) grad_w_in column c, K grad_b_in, K + 1 + m grad_w_mid[m], K + 1 + n_mid + m
// grad_b_mid[m], K + 1 + 2 n_mid grad_w_out -- D floats each -- then sum g at F D (padded to 16 bytes)
constexpr int64_t mlp_bwd_fields(int kin, int n_mid) { return kin + 2 + 2 * n_mid; }
constexpr int64_t mlp_bwd_part_floats(int kin, int n_mid, int log2d) { return (mlp_bwd_fields(kin, n_mid) << log2d) + 4; }

inline bool mlp_bwd_supported(int kin, int n_mid, int log2d)
{
    return mlp_supported(kin, n_mid, log2d) && n_mid <= MLP_BWD_MAX_MID && log2d <= MLP_BWD_MAX_LOG2D;
}

// relu: the act bits (ACT at those boundaries)
template <int LOG2D, int KIN, int NMID, bool TAIL, typename ACT = MlpRelu>
__device__ __forceinline__ void mlp_bwd_rows(
    uint32_t r0, uint32_t b1, const float *__restrict__ x, const float *__restrict__ gs, float *__restrict__ gxs,
    const float *lw1, const float *lbi, const float *lmid, const float *lwo, uint32_t col, bool has_b_in, uint32_t mid_bias,
    uint32_t relu, float (&gwi)[MlpGeom<LOG2D>::C][4][KIN], float (&gbi)[MlpGeom<LOG2D>::C][4],
    float (&gwm)[NMID][MlpGeom<LOG2D>::C][4], float (&gbm)[NMID][MlpGeom<LOG2D>::C][4], float (&gwo)[MlpGeom<LOG2D>::C][4],
    float &gsum)
{
    using Gm = MlpGeom<LOG2D>;
    constexpr int D = Gm::D, L = Gm::L, C = Gm::C, R = MlpBwdGeom<LOG2D>::R;
    typedef float f4 __attribute__((ext_vector_type(4)));
    // ---- the forward, keeping every layer's output: hs[0] behind the first layer, hs[1 + m] behind square layer m
    float xv[R][KIN];
    mlp_load_x<KIN, R>(xv, x, r0, b1);
    float hs[NMID + 1][R][C][4];
    mlp_first_layer<LOG2D, KIN, R, ACT>(hs[0], xv, lw1, lbi, col, has_b_in, (relu & 1u) != 0);
    uint32_t mask[NMID];
#pragma unroll
    for (int m = 0; m < NMID; ++m) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < C; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) hs[m + 1][r][j][e] = hs[m][r][j][e];
        mlp_square_layer<LOG2D, R, !ACT::SMOOTH, ACT>(hs[m + 1], lmid + 2 * m * D, lmid + (2 * m + 1) * D, col, (mid_bias >> m) & 1u,
                                                      (relu >> (m + 1)) & 1u, &mask[m]);
    }
    float gv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) gv[r] = gs[r0 + r < b1 ? r0 + r : b1 - 1];
    // ---- backward, element by element
    float gx[R][KIN];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < KIN; ++c) gx[r][c] = 0.0f;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const uint32_t q = col + j * L;
        const f4 wo = reinterpret_cast<const f4 *>(lwo)[q];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (TAIL && r0 + r >= b1) continue;                 // a clamped duplicate row: computed, never summed
            if (j == 0 && col == 0) gsum = gsum + gv[r];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float d = gv[r] * wo[e];                          // RowDotFunction: grad_x = g * w
                gwo[j][e] = __builtin_fmaf(hs[NMID][r][j][e], gv[r], gwo[j][e]);
#pragma unroll
                for (int m = NMID - 1; m >= 0; --m) {
                    if constexpr (ACT::SMOOTH) {
                        if ((relu >> (m + 1)) & 1u) d = ACT::bwd(d, hs[m + 1][r][j][e]);
                    } else {
                        if (((relu >> (m + 1)) & 1u) && !((mask[m] >> ((r * C + j) * 4 + e)) & 1u)) d = 0.0f;
                    }
                    gwm[m][j][e] = __builtin_fmaf(d, hs[m][r][j][e], gwm[m][j][e]);
                    gbm[m][j][e] = gbm[m][j][e] + d;
                    d = d * lmid[2 * m * D + 4 * q + e];
                }
                if (relu & 1u) {
                    if constexpr (ACT::SMOOTH) {
                        d = ACT::bwd(d, hs[0][r][j][e]);
                    } else if constexpr (KIN == 1) {
                        if (hs[0][r][j][e] <= 0.0f) d = 0.0f;     // the square layer's relu_in: NaN passes
                    } else {
                        d = d * (hs[0][r][j][e] > 0.0f ? 1.0f : 0.0f);   // SmallKApplyFunction: g * (out > 0)
                    }
                }
                gbi[j][e] = gbi[j][e] + d;
#pragma unroll
                for (int c = 0; c < KIN; ++c) {
                    gwi[j][e][c] = __builtin_fmaf(d, xv[r][c], gwi[j][e][c]);
                    if (gxs != nullptr) gx[r][c] = __builtin_fmaf(d, lw1[c * D + 4 * q + e], gx[r][c]);
                }
            }
        }
    }
    if (gxs != nullptr) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float out = 0.0f;
#pragma unroll
            for (int c = 0; c < KIN; ++c) {
                float v = gx[r][c];
#pragma unroll
                for (int m = 1; m < L; m <<= 1) v = v + __shfl_xor(v, m, 64);
                if (col == (uint32_t)c) out = v;
            }
            if (col < (uint32_t)KIN && (!TAIL || r0 + r < b1)) gxs[(size_t)(r0 + r) * KIN + col] = out;
        }
    }
}

// g : (S, B); gx : (S, B, KIN) or NULL; part : (S * n_slabs) blocks of mlp_bwd_part_floats floats.  Operands as mlp_apply_kernel;
// relu: the act bits (ACT at those boundaries).  TWIN: mlp_apply_bwd_kernel below repeats this body statement for statement
// with ACT = MlpRelu (see mlp_apply_kernel for why); a change to one -- tails, the LDS reduction, the slab layout -- must be
// made in both.
template <int LOG2D, int KIN, int NMID, typename ACT>
__device__ __forceinline__ void
mlp_apply_bwd_block(float *__restrict__ part, float *__restrict__ gx, const float *__restrict__ g,
                    const float *__restrict__ x, const float *__restrict__ w_in, const float *__restrict__ b_in,
                    const float *__restrict__ s1, const float *__restrict__ s2, const float *__restrict__ u,
                    const float *__restrict__ b_mid, const float *__restrict__ w_out, uint32_t S, uint32_t B, uint32_t mid_bias,
                    uint32_t relu, uint32_t slab_rows, uint32_t n_slabs)
{
    using Gm = MlpGeom<LOG2D>;
    constexpr int D = Gm::D, L = Gm::L, G = Gm::G, C = Gm::C, RPI = MlpBwdGeom<LOG2D>::RPI;
    constexpr int F = (int)mlp_bwd_fields(KIN, NMID);
    extern __shared__ __attribute__((aligned(16))) float mlp_lds[];
    float *lw1 = mlp_lds, *lbi = lw1 + KIN * D, *lmid = lbi + D, *lwo = lmid + 2 * NMID * D;

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t b0 = slab * slab_rows, b1 = b0 + slab_rows < B ? b0 + slab_rows : B;
    mlp_stage_operands<LOG2D, KIN>(mlp_lds, s, w_in, b_in, s1, s2, u, b_mid, w_out, S, NMID, mid_bias);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t grp = (uint32_t)lane / L, col = (uint32_t)lane % L;
    const bool has_b_in = b_in != nullptr;
    float gwi[C][4][KIN], gbi[C][4], gwm[NMID][C][4], gbm[NMID][C][4], gwo[C][4], gsum = 0.0f;
#pragma unroll
    for (int j = 0; j < C; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int c = 0; c < KIN; ++c) gwi[j][e][c] = 0.0f;
            gbi[j][e] = gwo[j][e] = 0.0f;
#pragma unroll
            for (int m = 0; m < NMID; ++m) gwm[m][j][e] = gbm[m][j][e] = 0.0f;
        }
    const float *gs = g + (size_t)s * B;
    float *gxs = gx != nullptr ? gx + (size_t)s * B * KIN : nullptr;
    for (uint32_t rb = b0 + wave * RPI; rb < b1; rb += 4 * RPI) {
        // D = 1024: re-read the operands from LDS on every iteration instead of letting them be hoisted into registers (as many
        // as the accumulators: 366 instead of 2xx VGPRs at K = 4, and a spill at K = 8 with two square layers)
        if constexpr (C >= 4) asm volatile("" ::: "memory");
        const uint32_t r0 = rb + grp * MlpBwdGeom<LOG2D>::R;
        if (rb + RPI <= b1)
            mlp_bwd_rows<LOG2D, KIN, NMID, false, ACT>(r0, b1, x, gs, gxs, lw1, lbi, lmid, lwo, col, has_b_in, mid_bias, relu, gwi,
                                                       gbi, gwm, gbm, gwo, gsum);
        else
            mlp_bwd_rows<LOG2D, KIN, NMID, true, ACT>(r0, b1, x, gs, gxs, lw1, lbi, lmid, lwo, col, has_b_in, mid_bias, relu, gwi,
                                                      gbi, gwm, gbm, gwo, gsum);
    }

    // ---- the block's sums: lane groups of a wave by a butterfly, then the waves through LDS in wave order
    auto each = [&](auto &&fn) {
#pragma unroll
        for (int j = 0; j < C; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t n = 4 * (col + j * L) + e;
#pragma unroll
                for (int c = 0; c < KIN; ++c) fn(gwi[j][e][c], c * D + n);
                fn(gbi[j][e], KIN * D + n);
#pragma unroll
                for (int m = 0; m < NMID; ++m) {
                    fn(gwm[m][j][e], (KIN + 1 + m) * D + n);
                    fn(gbm[m][j][e], (KIN + 1 + NMID + m) * D + n);
                }
                fn(gwo[j][e], (KIN + 1 + 2 * NMID) * D + n);
            }
        fn(gsum, F * D);
    };
    if constexpr (G > 1) {
        each([&](float &v, uint32_t) {
#pragma unroll
            for (int m = L; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
        });
    }
    __syncthreads();                                       // every wave is done with the operands: the LDS holds the sums now
    float *red = mlp_lds;
    for (int w = 0; w < 4; ++w) {
        if (wave == w && grp == 0) {
            each([&](float &v, uint32_t i) {
                if (i == (uint32_t)(F * D) && col != 0) return;
                red[i] = w == 0 ? v : red[i] + v;
            });
        }
        __syncthreads();
    }
    float *p = part + (size_t)blockIdx.x * mlp_bwd_part_floats(KIN, NMID, LOG2D);
    for (uint32_t i = threadIdx.x; i <= (uint32_t)(F * D); i += 256) p[i] = red[i];
}

// The ReLU backward, with a body of its own for the reason mlp_apply_kernel has one (mlp_apply.hpp).  TWIN of
// mlp_apply_bwd_block: a change to one must be made in both.
template <typename T, int LOG2D, int KIN, int NMID>
__global__ void __launch_bounds__(256)
mlp_apply_bwd_kernel(float *__restrict__ part, float *__restrict__ gx, const float *__restrict__ g, const float *__restrict__ x,
                     const float *__restrict__ w_in, const float *__restrict__ b_in, const float *__restrict__ s1,
                     const float *__restrict__ s2, const float *__restrict__ u, const float *__restrict__ b_mid,
                     const float *__restrict__ w_out, uint32_t S, uint32_t B, uint32_t mid_bias, uint32_t relu,
                     uint32_t slab_rows, uint32_t n_slabs)
{
    using Gm = MlpGeom<LOG2D>;
    constexpr int D = Gm::D, L = Gm::L, G = Gm::G, C = Gm::C, RPI = MlpBwdGeom<LOG2D>::RPI;
    constexpr int F = (int)mlp_bwd_fields(KIN, NMID);
    extern __shared__ __attribute__((aligned(16))) float mlp_lds[];
    float *lw1 = mlp_lds, *lbi = lw1 + KIN * D, *lmid = lbi + D, *lwo = lmid + 2 * NMID * D;

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t b0 = slab * slab_rows, b1 = b0 + slab_rows < B ? b0 + slab_rows : B;
    mlp_stage_operands<LOG2D, KIN>(mlp_lds, s, w_in, b_in, s1, s2, u, b_mid, w_out, S, NMID, mid_bias);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t grp = (uint32_t)lane / L, col = (uint32_t)lane % L;
    const bool has_b_in = b_in != nullptr;
    float gwi[C][4][KIN], gbi[C][4], gwm[NMID][C][4], gbm[NMID][C][4], gwo[C][4], gsum = 0.0f;
#pragma unroll
    for (int j = 0; j < C; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int c = 0; c < KIN; ++c) gwi[j][e][c] = 0.0f;
            gbi[j][e] = gwo[j][e] = 0.0f;
#pragma unroll
            for (int m = 0; m < NMID; ++m) gwm[m][j][e] = gbm[m][j][e] = 0.0f;
        }
    const float *gs = g + (size_t)s * B;
    float *gxs = gx != nullptr ? gx + (size_t)s * B * KIN : nullptr;
    for (uint32_t rb = b0 + wave * RPI; rb < b1; rb += 4 * RPI) {
        // D = 1024: re-read the operands from LDS on every iteration instead of letting them be hoisted into registers (as many
        // as the accumulators: 366 instead of 2xx VGPRs at K = 4, and a spill at K = 8 with two square layers)
        if constexpr (C >= 4) asm volatile("" ::: "memory");
        const uint32_t r0 = rb + grp * MlpBwdGeom<LOG2D>::R;
        if (rb + RPI <= b1)
            mlp_bwd_rows<LOG2D, KIN, NMID, false>(r0, b1, x, gs, gxs, lw1, lbi, lmid, lwo, col, has_b_in, mid_bias, relu, gwi, gbi,
                                                  gwm, gbm, gwo, gsum);
        else
            mlp_bwd_rows<LOG2D, KIN, NMID, true>(r0, b1, x, gs, gxs, lw1, lbi, lmid, lwo, col, has_b_in, mid_bias, relu, gwi, gbi,
                                                 gwm, gbm, gwo, gsum);
    }

    // ---- the block's sums: lane groups of a wave by a butterfly, then the waves through LDS in wave order
    auto each = [&](auto &&fn) {
#pragma unroll
        for (int j = 0; j < C; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t n = 4 * (col + j * L) + e;
#pragma unroll
                for (int c = 0; c < KIN; ++c) fn(gwi[j][e][c], c * D + n);
                fn(gbi[j][e], KIN * D + n);
#pragma unroll
                for (int m = 0; m < NMID; ++m) {
                    fn(gwm[m][j][e], (KIN + 1 + m) * D + n);
                    fn(gbm[m][j][e], (KIN + 1 + NMID + m) * D + n);
                }
                fn(gwo[j][e], (KIN + 1 + 2 * NMID) * D + n);
            }
        fn(gsum, F * D);
    };
    if constexpr (G > 1) {
        each([&](float &v, uint32_t) {
#pragma unroll
            for (int m = L; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
        });
    }
    __syncthreads();                                       // every wave is done with the operands: the LDS holds the sums now
    float *red = mlp_lds;
    for (int w = 0; w < 4; ++w) {
        if (wave == w && grp == 0) {
            each([&](float &v, uint32_t i) {
                if (i == (uint32_t)(F * D) && col != 0) return;
                red[i] = w == 0 ? v : red[i] + v;
            });
        }
        __syncthreads();
    }
    float *p = part + (size_t)blockIdx.x * mlp_bwd_part_floats(KIN, NMID, LOG2D);
    for (uint32_t i = threadIdx.x; i <= (uint32_t)(F * D); i += 256) p[i] = red[i];
}

// the backward of mlp_smooth_apply_kernel: ACT = WHVI_MLP_ACT_SIGMOID / _TANH at the boundaries of `act`
template <typename T, int LOG2D, int KIN, int NMID, int ACT>
__global__ void __launch_bounds__(256)
mlp_smooth_apply_bwd_kernel(float *__restrict__ part, float *__restrict__ gx, const float *__restrict__ g,
                            const float *__restrict__ x, const float *__restrict__ w_in, const float *__restrict__ b_in,
                            const float *__restrict__ s1, const float *__restrict__ s2, const float *__restrict__ u,
                            const float *__restrict__ b_mid, const float *__restrict__ w_out, uint32_t S, uint32_t B,
                            uint32_t mid_bias, uint32_t act, uint32_t slab_rows, uint32_t n_slabs)
{
    static_assert(MlpAct<ACT>::type::SMOOTH, "the ReLU backward is mlp_apply_bwd_kernel");
    mlp_apply_bwd_block<LOG2D, KIN, NMID, typename MlpAct<ACT>::type>(part, gx, g, x, w_in, b_in, s1, s2, u, b_mid, w_out,
                                                                       S, B, mid_bias, act, slab_rows, n_slabs);
}

// The finishing launch (mlp_apply_bwd_finish_kernel, defined once in mlp_apply_bwd.hip): the slabs' partial sums in `work` into
// the gradients, in ascending slab and sample order
int mlp_apply_bwd_finish(void *grad_w_in, void *grad_w_mid, void *grad_w_out, void *grad_b, const void *work, int64_t S,
                         int64_t n_slabs, int32_t first, int32_t n_mid, int32_t log2d, hipStream_t st);

// slabs per sample: about two blocks per CU over all samples, at least 256 rows (4 waves x 4 iterations of the widest group)
inline int64_t mlp_bwd_slabs(int64_t S, int64_t B)
{
    if (S < 1 || B < 1) return 1;
    int64_t n = (2 * (int64_t)num_cu() + S - 1) / S;
    const int64_t most = (B + 255) / 256;
    if (n > most) n = most;
    if (n < 1) n = 1;
    const int64_t slab_rows = (B + n - 1) / n;
    return (B + slab_rows - 1) / slab_rows;
}

// The launch of one call, from mlp_apply_bwd_check
struct MlpBwdLaunch {
    dim3 grid;
    size_t lds;
    uint32_t slab_rows, n_slabs;
};

// Every argument check of whvi_mlp_apply_bwd_f32 / whvi_mlp_apply_act_bwd_f32, before any launch; `bits` (named `bits_name` in
// the message) are the activation bits.  B = 0 zero-fills the gradients here.  WHVI_OK with ln.grid.x = 0: nothing to launch.
inline int mlp_apply_bwd_check(MlpBwdLaunch &ln, void *grad_w_in, void *grad_w_mid, void *grad_w_out, void *grad_b, void *grad_x,
                               void *work, int64_t work_floats, const void *g, const void *x, int32_t first, const void *w_in,
                               const void *b_in, int32_t n_mid, const void *s1, const void *s2, const void *u,
                               const void *b_mid, int32_t mid_bias, const void *w_out, int64_t S, int64_t B, int32_t log2d,
                               int32_t bits, const char *bits_name, hipStream_t st)
{
    ln.grid = dim3(0);
    if (S < 0 || B < 0) return fail(WHVI_ERR_ARG, "whvi_mlp_apply_bwd: negative size%s", "");
    if (first != WHVI_MLP_FIRST_COLUMN && first != WHVI_MLP_FIRST_K4 && first != WHVI_MLP_FIRST_K8)
        return fail(WHVI_ERR_ARG, "whvi_mlp_apply_bwd: unknown first-layer kind%s %lld", "", first);
    if (!mlp_bwd_supported(first, n_mid, log2d))
        return fail(WHVI_ERR_SIZE, "whvi_mlp_apply_bwd: unsupported network%s (n_mid = %lld, log2(D) = %lld; see "
                    "whvi_mlp_apply_bwd_supported)", "", n_mid, log2d);
    if (bits & ~((1 << (n_mid + 1)) - 1))
        return fail(WHVI_ERR_ARG, "whvi_mlp_apply_bwd: unknown %s bits 0x%llx", bits_name, bits);
    if (mid_bias & ~((1 << n_mid) - 1))
        return fail(WHVI_ERR_ARG, "whvi_mlp_apply_bwd: unknown mid_bias bits%s 0x%llx", "", mid_bias);
    if (S == 0) return WHVI_OK;
    if (S * B >= ((int64_t)1 << 32)) return fail(WHVI_ERR_SIZE, "whvi_mlp_apply_bwd: rows are indexed with 32 bits%s", "");
    if (S * (first + n_mid + 2) << log2d >= ((int64_t)1 << 31))
        return fail(WHVI_ERR_SIZE, "whvi_mlp_apply_bwd: gradients are indexed with 32 bits%s", "");
    if (!grad_w_in || !grad_w_mid || !grad_w_out || !grad_b || !w_in || !s1 || !s2 || !u || !w_out || (mid_bias != 0 && !b_mid) ||
        (B > 0 && (!work || !g || !x)))
        return fail(WHVI_ERR_ARG, "whvi_mlp_apply_bwd: null pointer%s", "");
    if (((uintptr_t)grad_w_in | (uintptr_t)grad_w_mid | (uintptr_t)grad_w_out | (uintptr_t)grad_x | (uintptr_t)work | (uintptr_t)x |
         (uintptr_t)w_in | (uintptr_t)b_in | (uintptr_t)s1 | (uintptr_t)s2 | (uintptr_t)u | (uintptr_t)b_mid | (uintptr_t)w_out) & 15)
        return fail(WHVI_ERR_ALIGN, "whvi_mlp_apply_bwd: a pointer%s is not 16-byte aligned", "");
    const int64_t n_slabs = mlp_bwd_slabs(S, B);
    const int64_t need = B > 0 ? S * n_slabs * mlp_bwd_part_floats(first, n_mid, log2d) : 0;
    if (work_floats < need)
        return fail(WHVI_ERR_ARG, "whvi_mlp_apply_bwd: workspace of%s %lld floats, %lld needed (whvi_mlp_apply_bwd_workspace)", "",
                    work_floats, need);
    const uint32_t D = 1u << log2d;
    if (B == 0) {                                          // no rows: every gradient is an empty sum
        const int64_t kin = first;
        const struct { void *p; int64_t n; } outs[] = {
            {grad_w_in, S * D * kin}, {grad_w_mid, n_mid * S * D}, {grad_w_out, S * D}, {grad_b, (1 + n_mid) * D + 1}};
        for (const auto &o : outs)
            if (hipMemsetAsync(o.p, 0, (size_t)o.n * 4, st) != hipSuccess) return fail(WHVI_ERR_LAUNCH, "whvi_mlp_apply_bwd: memset%s", "");
        return WHVI_OK;
    }
    const int64_t slab_rows = (B + n_slabs - 1) / n_slabs;
    if (n_slabs * S >= ((int64_t)1 << 31)) return fail(WHVI_ERR_SIZE, "whvi_mlp_apply_bwd: too many blocks%s", "");
    ln.lds = (size_t)mlp_lds_bytes(first, n_mid, log2d) + 16;
    ln.grid = dim3((unsigned)(n_slabs * S));
    ln.slab_rows = (uint32_t)slab_rows;
    ln.n_slabs = (uint32_t)n_slabs;
    return WHVI_OK;
}

inline int64_t mlp_apply_bwd_workspace(int64_t S, int64_t B, int32_t first, int32_t n_mid, int32_t log2d)
{
    if (S < 0 || B < 0 || !mlp_bwd_supported(first, n_mid, log2d)) return -1;
    if (S == 0 || B == 0) return 0;
    return S * mlp_bwd_slabs(S, B) * mlp_bwd_part_floats(first, n_mid, log2d);
}

}  // namespace whvi
