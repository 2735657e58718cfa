#pragma once
// whvi_amd/csrc/mlp_fastfood_apply_bwd.hpp -- backward of whvi_mlp_fastfood_apply_f32 (mlp_fastfood_apply.hip): the parameter
// gradients of a WHVI regression network with fastfood square layers for ALL Monte-Carlo samples from g = dL/dy, without any
// saved activation.
//
// Built like mlp_apply_bwd.hpp.  A block owns (sample s, a slab of batch rows), stages the sample's operands in LDS exactly as
// the forward does (mlp_ff_stage_operands) and recomputes each row's hidden vectors with the forward's arithmetic
// (mlp_first_layer; mlp_ff_layer_keep = mlp_ff_layer's statements, also handing back both transforms), so every activation
// output and ReLU sign is the forward's, bit for bit.  Geometry: MlpBwdGeom's R x C = 4 chunks per lane (16 hidden floats per
// vector); the transforms are fwht_tile with mlp_ff_layer's template arguments -- butterflies are per row, so the smaller R
// changes no value.  It then runs the batched route's backward formulas, last layer first:
//   output layer (RowDotFunction)   d = g * w_out;  grad_w_out += h_L * g
//   fastfood layer m, input h, t1 = H(s2 h), t2 = H(g_k t1), z = s1 t2 (+ bias)   (FastfoodFunction.backward; H is symmetric)
//                                   d = act'(.) d;  grad_bias += d;  grad_s1 += d t2;  v = H(s1 d);  grad_g[k] += v t1;
//                                   w = H(g_k v);  grad_s2 += w h;  d = s2 w
//                                   t1, t2 come from the kept layer input: the last layer's from the forward recompute itself,
//                                   an earlier layer's by running its two transforms again.  t1 and v both carry fwht_tile's
//                                   lane-sign convention SIGN_MID, which cancels in their product.
//   first layer                     d = act'(.) d;  grad_b_in += d;  grad_w_in[n, c] += d * x[c];
//                                   grad_x[s, b, c] = sum_n d * w_in[n, c] (a butterfly over the row's lanes)
// Activation backward, per boundary what the batched route runs there for a fastfood network:
//   sigmoid / tanh                  torch's formulas on the recomputed output (MlpSigmoid::bwd, MlpTanh::bwd)
//   ReLU in front of the output layer   folded into the row-dot launch (RowDotFunction, relu_in):   d = d * (out > 0)
//   ReLU behind a stacked first layer   folded into its launch (SmallKApplyFunction, relu_out):     d = d * (out > 0)
//   every other ReLU                an nn.ReLU module (threshold_backward): d = 0 where out <= 0, NaN passes
//                                   -- behind a column first layer, and between two fastfood layers, which fold nothing
// Each lane keeps the sums of its hidden units over its rows in registers, C * 4 * (K + 2 + 4 n_mid) floats -- the operands'
// field count, so the LDS that held the operands holds the block's reduction: lane groups of a wave combine by a butterfly,
// the four waves through LDS in wave order, and the block writes one partial per field to its slab of the workspace.  A second,
// tiny launch inside the same call (mlp_fastfood_apply_bwd_finish_kernel) adds the slabs in ascending order -- and, for s1,
// s2 and the biases, the samples: deterministic, no atomics, no allocation.
#include "mlp_apply_bwd.hpp"
#include "mlp_fastfood_apply.hpp"

namespace whvi {

// partial sums per block: fields [0, K) grad_w_in column c, K grad_b_in, then per square layer m at K + 1 + 4 m: grad_s2,
// grad_g, grad_s1, grad_bias (the order of the operands in LDS), K + 1 + 4 n_mid grad_w_out -- D floats each -- then sum g at
// F D (padded to 16 bytes)
constexpr int64_t mlp_ff_bwd_fields(int kin, int n_mid) { return kin + 2 + 4 * n_mid; }
constexpr int64_t mlp_ff_bwd_part_floats(int kin, int n_mid, int log2d) { return (mlp_ff_bwd_fields(kin, n_mid) << log2d) + 4; }

inline bool mlp_ff_bwd_supported(int kin, int n_mid, int log2d)
{
    return mlp_ff_supported(kin, n_mid, log2d) && n_mid <= MLP_BWD_MAX_MID && log2d <= MLP_BWD_MAX_LOG2D;
}

// dst = v (.) src for the lane's chunks: mlp_ff_scale's product (one rounding per element), into a second vector
template <int LOG2D, int R>
__device__ __forceinline__ void mlp_ff_scale_to(float (&dst)[R][MlpGeom<LOG2D>::C][4], const float (&src)[R][MlpGeom<LOG2D>::C][4],
                                                const float *lv, uint32_t col)
{
    using Gm = MlpGeom<LOG2D>;
    constexpr int L = Gm::L, C = Gm::C;
    typedef float f4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const f4 v = reinterpret_cast<const f4 *>(lv)[col + j * L];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[r][j][e] = v[e] * src[r][j][e];
    }
}

// the two transforms of a fastfood layer, as mlp_ff_layer issues them: FIRST from sign mask 0 (leaves SIGN_MID), the second
// from SIGN_MID (leaves 0)
template <int LOG2D, int R, bool FIRST>
__device__ __forceinline__ void mlp_ff_fwht(float (&h)[R][MlpGeom<LOG2D>::C][4], int lane)
{
    constexpr int K = R * MlpGeom<LOG2D>::C;
    constexpr int SIGN_MID = fwht_sign_out<4, LOG2D>(0);
    static_assert(fwht_sign_out<4, LOG2D>(SIGN_MID) == 0, "two transforms restore the sign convention");
    float (&t)[K][4] = reinterpret_cast<float (&)[K][4]>(h);          // chunk (r, j) = tile chunk k = r C + j
    if constexpr (FIRST) fwht_tile<float, 4, K, LOG2D, POLICY_DPP, FUSED_PKMASK, true, 0>(t, lane);
    else fwht_tile<float, 4, K, LOG2D, POLICY_DPP, FUSED_PKMASK, true, SIGN_MID>(t, lane);
}

// mlp_ff_layer out of place, keeping both transforms: t1 = H(s2 hin) (sign convention SIGN_MID), t2 = H(g_k t1),
// out = act(s1 t2 (+ bias)).  The same statements in the same order: the same bits.
template <int LOG2D, int R, typename ACT>
__device__ __forceinline__ void mlp_ff_layer_keep(float (&out)[R][MlpGeom<LOG2D>::C][4], float (&t1)[R][MlpGeom<LOG2D>::C][4],
                                                  float (&t2)[R][MlpGeom<LOG2D>::C][4], const float (&hin)[R][MlpGeom<LOG2D>::C][4],
                                                  const float *lop, int lane, uint32_t col, bool hb, bool ha)
{
    using Gm = MlpGeom<LOG2D>;
    constexpr int D = Gm::D, L = Gm::L, C = Gm::C;
    typedef float f4 __attribute__((ext_vector_type(4)));
    mlp_ff_scale_to<LOG2D, R>(t1, hin, lop, col);
    mlp_ff_fwht<LOG2D, R, true>(t1, lane);
    mlp_ff_scale_to<LOG2D, R>(t2, t1, lop + D, col);
    mlp_ff_fwht<LOG2D, R, false>(t2, lane);
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const uint32_t q = col + j * L;
        const f4 a = reinterpret_cast<const f4 *>(lop + 2 * D)[q];
        const f4 bc = reinterpret_cast<const f4 *>(lop + 3 * D)[q];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = a[e] * t2[r][j][e];
                if (hb) v = v + bc[e];
                if (ha) v = ACT::fwd(v);
                out[r][j][e] = v;
            }
    }
}

// The rows r0 .. r0 + R - 1 of one lane group: forward recompute, then the backward.  act: the act bits (ACT at those
// boundaries).  TAIL: rows past b1 are clamped duplicates -- computed (every lane takes part in the transforms), never summed.
template <int LOG2D, int KIN, int NMID, bool TAIL, typename ACT>
__device__ __forceinline__ void mlp_ff_bwd_rows(
    uint32_t r0, uint32_t b1, const float *__restrict__ x, const float *__restrict__ gs, float *__restrict__ gxs,
    const float *lw1, const float *lbi, const float *lwo, const float *lff, int lane, uint32_t col, bool has_b_in,
    uint32_t mid_bias, uint32_t act, float (&gwi)[MlpGeom<LOG2D>::C][4][KIN], float (&gbi)[MlpGeom<LOG2D>::C][4],
    float (&gff)[NMID][4][MlpGeom<LOG2D>::C][4], float (&gwo)[MlpGeom<LOG2D>::C][4], float &gsum)
{
    using Gm = MlpGeom<LOG2D>;
    constexpr int D = Gm::D, L = Gm::L, C = Gm::C, R = MlpBwdGeom<LOG2D>::R;
    typedef float f4 __attribute__((ext_vector_type(4)));
    // ---- the forward, keeping every layer's output: hs[0] behind the first layer, hs[1 + m] behind square layer m; t1, t2:
    // the last square layer's transforms
    float xv[R][KIN];
    mlp_load_x<KIN, R>(xv, x, r0, b1);
    float hs[NMID + 1][R][C][4], t1[R][C][4], t2[R][C][4];
    mlp_first_layer<LOG2D, KIN, R, ACT>(hs[0], xv, lw1, lbi, col, has_b_in, (act & 1u) != 0);
#pragma unroll
    for (int m = 0; m < NMID; ++m)
        mlp_ff_layer_keep<LOG2D, R, ACT>(hs[m + 1], t1, t2, hs[m], lff + 4 * m * D, lane, col, (mid_bias >> m) & 1u,
                                         (act >> (m + 1)) & 1u);
    float gv[R];
    bool ok[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        gv[r] = gs[r0 + r < b1 ? r0 + r : b1 - 1];
        ok[r] = !TAIL || r0 + r < b1;
    }
    // ---- output layer (RowDotFunction): d = g * w_out, grad_w_out += h_L * g
    float d[R][C][4];
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const f4 wo = reinterpret_cast<const f4 *>(lwo)[col + j * L];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (j == 0 && col == 0 && ok[r]) gsum = gsum + gv[r];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                d[r][j][e] = gv[r] * wo[e];
                if (ok[r]) gwo[j][e] = __builtin_fmaf(hs[NMID][r][j][e], gv[r], gwo[j][e]);
            }
        }
    }
    // ---- fastfood layers, last first
#pragma unroll
    for (int m = NMID - 1; m >= 0; --m) {
        const float *lop = lff + 4 * m * D;
        if (m != NMID - 1) {                                   // an earlier layer: its transforms again, from its kept input
            float unused[R][C][4];
            mlp_ff_layer_keep<LOG2D, R, ACT>(unused, t1, t2, hs[m], lop, lane, col, false, false);
        }
        const bool ha = (act >> (m + 1)) & 1u;
#pragma unroll
        for (int j = 0; j < C; ++j)
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v = d[r][j][e];
                    const float y = hs[m + 1][r][j][e];
                    if (ha) {
                        if constexpr (ACT::SMOOTH) v = ACT::bwd(v, y);
                        else if (m == NMID - 1) v = v * (y > 0.0f ? 1.0f : 0.0f);       // RowDotFunction's relu_in: g * (x > 0)
                        else if (y <= 0.0f) v = 0.0f;                                    // nn.ReLU's threshold_backward: NaN passes
                    }
                    d[r][j][e] = v;
                    if (ok[r]) {
                        gff[m][3][j][e] = gff[m][3][j][e] + v;                           // grad_bias
                        gff[m][2][j][e] = __builtin_fmaf(v, t2[r][j][e], gff[m][2][j][e]);   // grad_s1
                    }
                }
        mlp_ff_scale<LOG2D, R>(d, lop + 2 * D, col);                                     // v = H(s1 d)
        mlp_ff_fwht<LOG2D, R, true>(d, lane);
#pragma unroll
        for (int j = 0; j < C; ++j)
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (ok[r]) gff[m][1][j][e] = __builtin_fmaf(d[r][j][e], t1[r][j][e], gff[m][1][j][e]);   // grad_g[k]
        mlp_ff_scale<LOG2D, R>(d, lop + D, col);                                         // w = H(g_k v)
        mlp_ff_fwht<LOG2D, R, false>(d, lane);
#pragma unroll
        for (int j = 0; j < C; ++j)
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (ok[r]) gff[m][0][j][e] = __builtin_fmaf(d[r][j][e], hs[m][r][j][e], gff[m][0][j][e]);   // grad_s2
        mlp_ff_scale<LOG2D, R>(d, lop, col);                                             // d = s2 w
    }
    // ---- first layer
    float gx[R][KIN];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < KIN; ++c) gx[r][c] = 0.0f;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const uint32_t q = col + j * L;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = d[r][j][e];
                const float y = hs[0][r][j][e];
                if (act & 1u) {
                    if constexpr (ACT::SMOOTH) {
                        v = ACT::bwd(v, y);
                    } else if constexpr (KIN == 1) {
                        if (y <= 0.0f) v = 0.0f;                   // the column layer's nn.ReLU: NaN passes
                    } else {
                        v = v * (y > 0.0f ? 1.0f : 0.0f);          // SmallKApplyFunction: g * (out > 0)
                    }
                }
                if (ok[r]) gbi[j][e] = gbi[j][e] + v;
#pragma unroll
                for (int c = 0; c < KIN; ++c) {
                    if (ok[r]) gwi[j][e][c] = __builtin_fmaf(v, xv[r][c], gwi[j][e][c]);
                    if (gxs != nullptr) gx[r][c] = __builtin_fmaf(v, lw1[c * D + 4 * q + e], gx[r][c]);
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
            if (col < (uint32_t)KIN && ok[r]) gxs[(size_t)(r0 + r) * KIN + col] = out;
        }
    }
}

// g : (S, B); gx : (S, B, KIN) or NULL; part : (S * n_slabs) blocks of mlp_ff_bwd_part_floats floats.  Operands as
// mlp_fastfood_apply_kernel; ACT: WHVI_MLP_ACT_*.
template <typename T, int LOG2D, int KIN, int NMID, int ACT>      // (T = float; named so that whvi_last_kernel prints the real symbol)
__global__ void __launch_bounds__(256)
mlp_fastfood_apply_bwd_kernel(float *__restrict__ part, float *__restrict__ gx, const float *__restrict__ g,
                              const float *__restrict__ x, const float *__restrict__ w_in, const float *__restrict__ b_in,
                              const float *__restrict__ s1, const float *__restrict__ s2, const float *__restrict__ gk,
                              const float *__restrict__ b_mid, const float *__restrict__ w_out, uint32_t S, uint32_t B,
                              uint32_t mid_bias, uint32_t act, uint32_t slab_rows, uint32_t n_slabs)
{
    using Gm = MlpGeom<LOG2D>;
    using Act = typename MlpAct<ACT>::type;
    constexpr int D = Gm::D, L = Gm::L, G = Gm::G, C = Gm::C, RPI = MlpBwdGeom<LOG2D>::RPI;
    constexpr int F = (int)mlp_ff_bwd_fields(KIN, NMID);
    extern __shared__ __attribute__((aligned(16))) float mlp_lds[];
    float *lw1 = mlp_lds, *lbi = lw1 + KIN * D, *lwo = lbi + D, *lff = lwo + D;

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t b0 = slab * slab_rows, b1 = b0 + slab_rows < B ? b0 + slab_rows : B;
    mlp_ff_stage_operands<LOG2D, KIN>(mlp_lds, s, w_in, b_in, s1, s2, gk, b_mid, w_out, S, NMID, mid_bias);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t grp = (uint32_t)lane / L, col = (uint32_t)lane % L;
    const bool has_b_in = b_in != nullptr;
    float gwi[C][4][KIN], gbi[C][4], gff[NMID][4][C][4], gwo[C][4], gsum = 0.0f;
#pragma unroll
    for (int j = 0; j < C; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int c = 0; c < KIN; ++c) gwi[j][e][c] = 0.0f;
            gbi[j][e] = gwo[j][e] = 0.0f;
#pragma unroll
            for (int m = 0; m < NMID; ++m)
#pragma unroll
                for (int f = 0; f < 4; ++f) gff[m][f][j][e] = 0.0f;
        }
    const float *gs = g + (size_t)s * B;
    float *gxs = gx != nullptr ? gx + (size_t)s * B * KIN : nullptr;
    // the loop bound is wave-uniform: every lane of the wave takes part in the DPP / permlane stages of the transforms
    for (uint32_t rb = b0 + wave * RPI; rb < b1; rb += 4 * RPI) {
        // D = 1024: re-read the operands from LDS on every iteration rather than hoisting them into registers (mlp_apply_bwd.hpp)
        if constexpr (C >= 4) asm volatile("" ::: "memory");
        const uint32_t r0 = rb + grp * MlpBwdGeom<LOG2D>::R;
        if (rb + RPI <= b1)
            mlp_ff_bwd_rows<LOG2D, KIN, NMID, false, Act>(r0, b1, x, gs, gxs, lw1, lbi, lwo, lff, lane, col, has_b_in, mid_bias, act,
                                                          gwi, gbi, gff, gwo, gsum);
        else
            mlp_ff_bwd_rows<LOG2D, KIN, NMID, true, Act>(r0, b1, x, gs, gxs, lw1, lbi, lwo, lff, lane, col, has_b_in, mid_bias, act,
                                                         gwi, gbi, gff, gwo, gsum);
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
                for (int m = 0; m < NMID; ++m)
#pragma unroll
                    for (int f = 0; f < 4; ++f) fn(gff[m][f][j][e], (KIN + 1 + 4 * m + f) * D + n);
                fn(gwo[j][e], (KIN + 1 + 4 * NMID) * D + n);
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
    float *p = part + (size_t)blockIdx.x * mlp_ff_bwd_part_floats(KIN, NMID, LOG2D);
    for (uint32_t i = threadIdx.x; i <= (uint32_t)(F * D); i += 256) p[i] = red[i];
}

// The launch of one call, from mlp_ff_bwd_check
struct MlpFfBwdArgs {
    void *grad_x, *work;
    const void *g, *x, *w_in, *b_in, *s1, *s2, *gk, *b_mid, *w_out;
    int32_t first, n_mid, mid_bias, log2d, act_bits;
    int64_t S, B;
    MlpBwdLaunch ln;
};

// the backward launch for one activation kind; each is defined where its instantiations are compiled
// (mlp_fastfood_apply_bwd.hip: ReLU; mlp_fastfood_smooth_apply_bwd.hip: sigmoid and tanh)
void mlp_ff_bwd_launch_relu(const MlpFfBwdArgs &a, hipStream_t st);
void mlp_ff_bwd_launch_sigmoid(const MlpFfBwdArgs &a, hipStream_t st);
void mlp_ff_bwd_launch_tanh(const MlpFfBwdArgs &a, hipStream_t st);

template <int ACT, int L, int K, int N>
inline void mlp_ff_bwd_launch_one(const MlpFfBwdArgs &a, hipStream_t st)
{
    if constexpr (mlp_ff_lds_bytes(K, N, L) <= MLP_MAX_LDS) {
        note_launch<float>("mlp_fastfood_apply_bwd_kernel", L, K, N, ACT);
        hipLaunchKernelGGL((mlp_fastfood_apply_bwd_kernel<float, L, K, N, ACT>), a.ln.grid, dim3(256), a.ln.lds, st,
                           (float *)a.work, (float *)a.grad_x, (const float *)a.g, (const float *)a.x, (const float *)a.w_in,
                           (const float *)a.b_in, (const float *)a.s1, (const float *)a.s2, (const float *)a.gk,
                           (const float *)a.b_mid, (const float *)a.w_out, (uint32_t)a.S, (uint32_t)a.B, (uint32_t)a.mid_bias,
                           (uint32_t)a.act_bits, a.ln.slab_rows, a.ln.n_slabs);
    }
}

template <int ACT, int L>
inline void mlp_ff_bwd_launch_d(const MlpFfBwdArgs &a, hipStream_t st)
{
    if (a.first == 1) { if (a.n_mid == 1) mlp_ff_bwd_launch_one<ACT, L, 1, 1>(a, st); else mlp_ff_bwd_launch_one<ACT, L, 1, 2>(a, st); }
    else if (a.first == 4) { if (a.n_mid == 1) mlp_ff_bwd_launch_one<ACT, L, 4, 1>(a, st); else mlp_ff_bwd_launch_one<ACT, L, 4, 2>(a, st); }
    else { if (a.n_mid == 1) mlp_ff_bwd_launch_one<ACT, L, 8, 1>(a, st); else mlp_ff_bwd_launch_one<ACT, L, 8, 2>(a, st); }
}

// the definition of one of the three launch functions above
#define WHVI_MLP_FF_BWD_DEFINE(NAME, ACT)                                                                       \
    void NAME(const MlpFfBwdArgs &a, hipStream_t st)                                                            \
    {                                                                                                           \
        switch (a.log2d) {                                                                                      \
        case 6: mlp_ff_bwd_launch_d<ACT, 6>(a, st); break;                                                      \
        case 7: mlp_ff_bwd_launch_d<ACT, 7>(a, st); break;                                                      \
        case 8: mlp_ff_bwd_launch_d<ACT, 8>(a, st); break;                                                      \
        case 9: mlp_ff_bwd_launch_d<ACT, 9>(a, st); break;                                                      \
        case 10: mlp_ff_bwd_launch_d<ACT, 10>(a, st); break;                                                    \
        default: break;                                                                                         \
        }                                                                                                       \
    }

}  // namespace whvi
