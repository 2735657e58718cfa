#pragma once
// whvi_amd/csrc/mlp_fastfood_apply.hpp -- what the one-launch passes of a fastfood network share: the supported() rule, the
// staging of one sample's operands and the square layer (mlp_fastfood_apply.hip: the predictive pass;
// mlp_fastfood_apply_bwd.hpp: its backward, which recomputes the hidden vectors with these helpers).
#include "dispatch.hpp"
#include "fwht_tile.hpp"
#include "mlp_apply.hpp"

namespace whvi {

// LDS bytes of one sample's operands (the supported() rule; mirrored by whvi_amd/_hip.py)
constexpr int64_t mlp_ff_lds_bytes(int kin, int n_mid, int log2d) { return ((int64_t)4 << log2d) * (kin + 2 + 4 * n_mid); }

inline bool mlp_ff_supported(int kin, int n_mid, int log2d)
{
    return (kin == 1 || kin == 4 || kin == 8) && n_mid >= 1 && n_mid <= MLP_MAX_MID && log2d >= 6 && log2d <= 11 &&
           mlp_ff_lds_bytes(kin, n_mid, log2d) <= MLP_MAX_LDS;
}

// This sample's operands into the block's LDS: W1 transposed to [c][n], b_in, w_out, then per square layer m, at 4 m D:
// s2, g_k (row s of layer m's (S, D) block), s1, bias (zeros without one)
template <int LOG2D, int KIN>
__device__ __forceinline__ void mlp_ff_stage_operands(float *lds, uint32_t s, const float *__restrict__ w_in,
                                                      const float *__restrict__ b_in, const float *__restrict__ s1,
                                                      const float *__restrict__ s2, const float *__restrict__ g,
                                                      const float *__restrict__ b_mid, const float *__restrict__ w_out,
                                                      uint32_t S, uint32_t n_mid, uint32_t mid_bias)
{
    constexpr int D = 1 << LOG2D;
    typedef float f4 __attribute__((ext_vector_type(4)));
    float *lw1 = lds, *lbi = lw1 + KIN * D, *lwo = lbi + D, *lff = lwo + D;
    for (uint32_t n = threadIdx.x; n < (uint32_t)D; n += 256) {
        if constexpr (KIN == 1) {
            lw1[n] = w_in[(size_t)s * D + n];
        } else {
#pragma unroll
            for (int q = 0; q < KIN / 4; ++q) {
                const f4 v = reinterpret_cast<const f4 *>(w_in + ((size_t)s * D + n) * KIN)[q];
#pragma unroll
                for (int e = 0; e < 4; ++e) lw1[(4 * q + e) * D + n] = v[e];
            }
        }
        lbi[n] = b_in != nullptr ? b_in[n] : 0.0f;
        lwo[n] = w_out[(size_t)s * D + n];
    }
    for (uint32_t m = 0; m < n_mid; ++m) {
        f4 *l = reinterpret_cast<f4 *>(lff + 4 * m * D);
        for (uint32_t c = threadIdx.x; c < (uint32_t)D / 4; c += 256) {
            l[c] = reinterpret_cast<const f4 *>(s2 + (size_t)m * D)[c];
            l[D / 4 + c] = reinterpret_cast<const f4 *>(g + ((size_t)m * S + s) * D)[c];
            l[D / 2 + c] = reinterpret_cast<const f4 *>(s1 + (size_t)m * D)[c];
            l[3 * D / 4 + c] = ((mid_bias >> m) & 1u) ? reinterpret_cast<const f4 *>(b_mid + (size_t)m * D)[c] : f4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

// h = v (.) h for the lane's chunks (one rounding per element; v read from LDS chunk by chunk)
template <int LOG2D, int R>
__device__ __forceinline__ void mlp_ff_scale(float (&h)[R][MlpGeom<LOG2D>::C][4], const float *lv, uint32_t col)
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
            for (int e = 0; e < 4; ++e) h[r][j][e] = v[e] * h[r][j][e];
    }
}

// one fastfood layer in place: fused_shs_kernel's s2, FWHT, g_k, FWHT, s1 -- then + bias (hb) and the activation (ha).
// lop: the layer's LDS block (s2, g_k, s1, bias at 0, D, 2 D, 3 D).
template <int LOG2D, int R, typename ACT>
__device__ __forceinline__ void mlp_ff_layer(float (&h)[R][MlpGeom<LOG2D>::C][4], const float *lop, int lane, uint32_t col,
                                             bool hb, bool ha)
{
    using Gm = MlpGeom<LOG2D>;
    constexpr int D = Gm::D, L = Gm::L, C = Gm::C, K = R * C;
    // the fused kernel's transforms: the signed DPP network; the first leaves the tile with SIGN_MID, the second clears it
    constexpr int SIGN_MID = fwht_sign_out<4, LOG2D>(0);
    static_assert(fwht_sign_out<4, LOG2D>(SIGN_MID) == 0, "two transforms restore the sign convention");
    typedef float f4 __attribute__((ext_vector_type(4)));
    float (&t)[K][4] = reinterpret_cast<float (&)[K][4]>(h);          // chunk (r, j) = tile chunk k = r C + j
    mlp_ff_scale<LOG2D, R>(h, lop, col);
    fwht_tile<float, 4, K, LOG2D, POLICY_DPP, FUSED_PKMASK, true, 0>(t, lane);
    mlp_ff_scale<LOG2D, R>(h, lop + D, col);
    fwht_tile<float, 4, K, LOG2D, POLICY_DPP, FUSED_PKMASK, true, SIGN_MID>(t, lane);
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const uint32_t q = col + j * L;
        const f4 a = reinterpret_cast<const f4 *>(lop + 2 * D)[q];
        const f4 bc = reinterpret_cast<const f4 *>(lop + 3 * D)[q];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = a[e] * h[r][j][e];
                if (hb) v = v + bc[e];                     // torch's `out + self.bias`: a rounding of its own
                if (ha) v = ACT::fwd(v);
                h[r][j][e] = v;
            }
    }
}

}  // namespace whvi
