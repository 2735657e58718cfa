#pragma once
// whvi_amd/csrc/mlp_apply.hpp -- the predictive pass of a WHVI regression network of the canonical shape
//
//     WHVILinear(n_in, D) [ReLU] WHVILinear(D, D) [ReLU] ... WHVILinear(D, D) [ReLU] WHVILinear(D, 1)
//
// for ALL Monte-Carlo samples in ONE launch that keeps each row's hidden vector in registers: it reads x and writes y and
// nothing else (the three-launch route writes and re-reads two (S, B, D) activations).  Every stage repeats the arithmetic of
// the launch it replaces, in the same order, so the result is bit-identical to that route:
//   first layer, stacked (K = 4 / 8)  small_k_apply_kernel: a = +0; a = fmaf(x[b, c], W1[s, n, c], a) for c ascending (all K
//                                     products, exact zeros of the as-written weight included); + b_in; relu_
//   first layer, column (n_in = 1)    `x * w` of WHVIColumnMatrix: x[b, 0] * w[s, n] (no accumulator: -0 survives); + b_in; relu_
//   square layers                     diag_apply_kernel: row poison (a non-finite entry turns every OTHER entry of its row into
//                                     NaN), r * wbar_diag + 0, + b_mid, relu_ -- the diagonal from diag_apply.hpp's helpers
//   transposed column layer           row_dot_kernel: the same chunk -> lane map (D >= 256: lane l holds chunks l, l + 64, ...;
//                                     D < 256: D / 4 lanes per row), per-chunk x0 * w0 then fmaf, chunk partials in ascending
//                                     order, the same __shfl_xor butterfly, + b_out
// An nn.ReLU between two layers is relu_ (NaN passes) at that boundary wherever today's route applies it.  The smooth
// activations (mlp_smooth_apply_kernel, ACT = WHVI_MLP_ACT_SIGMOID / _TANH) run ATen's float formulas at the same places:
//   sigmoid  1.0f / (1.0f + expf(-z))    (ocml expf, IEEE division: sigmoid(+inf) = 1, sigmoid(-inf) = 0, NaN passes)
//   tanh     tanhf(z)                     (ocml; tanh(+-inf) = +-1, NaN passes)
// and, as on today's route, before the next square layer's row poison.
//
// Geometry: a block owns (sample s, a slab of batch rows).  It first stages that sample's operands in LDS -- W1 transposed to
// [c][n], b_in, per square layer its diagonal and bias, w_out: 4 D (K + 2 + 2 n_mid) bytes, at most 64 KiB -- then each wave
// walks row groups: a lane holds R rows x C chunks of the hidden vector (64 floats at D >= 512), reads every operand chunk from
// LDS once per R rows, and the R results of a lane group are stored by R neighbouring lanes.  No atomics, no scratch.
#include "dispatch.hpp"
#include "diag_apply.hpp"

namespace whvi {

constexpr int MLP_MAX_MID = 4;
constexpr int64_t MLP_MAX_LDS = (int64_t)64 * 1024;

// LDS bytes of one sample's operands (the supported() rule below; mirrored by whvi_amd/_hip.py)
constexpr int64_t mlp_lds_bytes(int kin, int n_mid, int log2d) { return ((int64_t)4 << log2d) * (kin + 2 + 2 * n_mid); }

inline bool mlp_supported(int kin, int n_mid, int log2d)
{
    return (kin == 1 || kin == 4 || kin == 8) && n_mid >= 1 && n_mid <= MLP_MAX_MID && log2d >= 6 && log2d <= 11 &&
           mlp_lds_bytes(kin, n_mid, log2d) <= MLP_MAX_LDS;
}

template <int LOG2D> struct MlpGeom {
    static constexpr int D = 1 << LOG2D;
    static constexpr int CPR = D / 4;                     // 16-byte chunks per row
    static constexpr int L = CPR < 64 ? CPR : 64;         // lanes per row (row_dot_kernel's layout)
    static constexpr int G = 64 / L;                      // rows side by side in one wave
    static constexpr int C = CPR / L;                     // chunks per lane and row: col, col + 64, ...
    static constexpr int R = C >= 4 ? 16 / C : 8;         // rows per lane group and iteration (R * C * 4 <= 64 hidden floats)
    static constexpr int RPI = G * R;                     // rows per wave iteration
};

// Activation policies of the fused passes.  fwd: the activation at a boundary; bwd(d, y): its gradient from the incoming
// gradient d and the activation's output y, torch's formula (sigmoid_backward / tanh_backward) in the same order.  The ReLU
// policy's backward is not a formula of y: its kernels recompute masks (mlp_square_layer<MASK>, mlp_bwd_rows).
struct MlpRelu {
    static constexpr bool SMOOTH = false;
    __device__ static __forceinline__ float fwd(float z) { return relu_(z); }
};
struct MlpSigmoid {
    static constexpr bool SMOOTH = true;
    __device__ static __forceinline__ float fwd(float z) { return 1.0f / (1.0f + expf(-z)); }          // ATen's sigmoid (float)
    __device__ static __forceinline__ float bwd(float d, float y) { return (d * (1.0f - y)) * y; }
};
struct MlpTanh {
    static constexpr bool SMOOTH = true;
    __device__ static __forceinline__ float fwd(float z) { return tanhf(z); }
    __device__ static __forceinline__ float bwd(float d, float y) { return d * (1.0f - y * y); }
};
// WHVI_MLP_ACT_* -> policy (the smooth kernels carry the ABI's number as their last template argument)
template <int ACT> struct MlpAct;
template <> struct MlpAct<WHVI_MLP_ACT_RELU> { using type = MlpRelu; };
template <> struct MlpAct<WHVI_MLP_ACT_SIGMOID> { using type = MlpSigmoid; };
template <> struct MlpAct<WHVI_MLP_ACT_TANH> { using type = MlpTanh; };

// diag_apply_kernel's row-poison rule for the R rows a lane group holds (rare path, behind a wave ballot)
template <int L, int R, int C>
__device__ __forceinline__ void mlp_poison_rows(float (&h)[R][C][4])
{
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t s = 0;
#pragma unroll
        for (int j = 0; j < C; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) s += __builtin_isfinite(h[r][j][e]) ? 0u : 1u;
#pragma unroll
        for (int m = 1; m < L; m <<= 1) s += (uint32_t)__shfl_xor((int)s, m, 64);      // the L lanes of the row
#pragma unroll
        for (int j = 0; j < C; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (s - (__builtin_isfinite(h[r][j][e]) ? 0u : 1u) != 0u) h[r][j][e] = __builtin_nan("");
    }
}

// This sample's operands into the block's LDS: W1 transposed to [c][n], b_in, per square layer its diagonal and bias, w_out.
// (Shared with the backward, mlp_apply_bwd.hpp, which recomputes the hidden vectors from the same copies.)
template <int LOG2D, int KIN>
__device__ __forceinline__ void mlp_stage_operands(float *lds, uint32_t s, const float *__restrict__ w_in,
                                                   const float *__restrict__ b_in, const float *__restrict__ s1,
                                                   const float *__restrict__ s2, const float *__restrict__ u,
                                                   const float *__restrict__ b_mid, const float *__restrict__ w_out,
                                                   uint32_t S, uint32_t n_mid, uint32_t mid_bias)
{
    constexpr int D = 1 << LOG2D;
    typedef float f4 __attribute__((ext_vector_type(4)));
    float *lw1 = lds, *lbi = lw1 + KIN * D, *lmid = lbi + D, *lwo = lmid + 2 * n_mid * D;
    for (uint32_t n = threadIdx.x; n < (uint32_t)D; n += 256) {
        if constexpr (KIN == 1) {
            lw1[n] = w_in[(size_t)s * D + n];
        } else {
#pragma unroll
            for (int g = 0; g < KIN / 4; ++g) {
                const f4 v = reinterpret_cast<const f4 *>(w_in + ((size_t)s * D + n) * KIN)[g];
#pragma unroll
                for (int e = 0; e < 4; ++e) lw1[(4 * g + e) * D + n] = v[e];
            }
        }
        lbi[n] = b_in != nullptr ? b_in[n] : 0.0f;
        lwo[n] = w_out[(size_t)s * D + n];
    }
    for (uint32_t m = 0; m < n_mid; ++m) {
        for (uint32_t c = threadIdx.x; c < (uint32_t)D / 4; c += 256) {
            float wv[4];
            diag_w_chunk<float, LOG2D>(s1 + (size_t)m * D, s2 + (size_t)m * D, u + (size_t)m * (S + 1) * D, s, 1u, c * 4, wv);
            reinterpret_cast<f4 *>(lmid + 2 * m * D)[c] = f4{wv[0], wv[1], wv[2], wv[3]};
            reinterpret_cast<f4 *>(lmid + (2 * m + 1) * D)[c] =
                ((mid_bias >> m) & 1u) ? reinterpret_cast<const f4 *>(b_mid + (size_t)m * D)[c] : f4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

// x[row, :] of the R rows r0 .. r0 + R - 1 (rows past b1 read row b1 - 1: valid operands, never stored)
template <int KIN, int R>
__device__ __forceinline__ void mlp_load_x(float (&xv)[R][KIN], const float *__restrict__ x, uint32_t r0, uint32_t b1)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t row = r0 + r < b1 ? r0 + r : b1 - 1;
        if constexpr (KIN == 1) {
            xv[r][0] = x[row];
        } else {
#pragma unroll
            for (int g = 0; g < KIN / 4; ++g) {
                const f4 v = reinterpret_cast<const f4 *>(x + (size_t)row * KIN)[g];
#pragma unroll
                for (int e = 0; e < 4; ++e) xv[r][4 * g + e] = v[e];
            }
        }
    }
}

// first layer: small_k_apply_kernel's +0-initialised fmaf chain (KIN = 4 / 8) or the column layer's plain product, + b_in,
// the activation (act0)
template <int LOG2D, int KIN, int R, typename ACT = MlpRelu>
__device__ __forceinline__ void mlp_first_layer(float (&h)[R][MlpGeom<LOG2D>::C][4], const float (&xv)[R][KIN], const float *lw1,
                                                const float *lbi, uint32_t col, bool has_b_in, bool act0)
{
    using Gm = MlpGeom<LOG2D>;
    constexpr int D = Gm::D, L = Gm::L, C = Gm::C;
    typedef float f4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const uint32_t q = col + j * L;
        f4 wc[KIN];
#pragma unroll
        for (int c = 0; c < KIN; ++c) wc[c] = reinterpret_cast<const f4 *>(lw1 + c * D)[q];
        const f4 bc = reinterpret_cast<const f4 *>(lbi)[q];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a;
                if constexpr (KIN == 1) {
                    a = xv[r][0] * wc[0][e];                       // `x * w`: one rounding, no accumulator
                } else {
                    a = 0.0f;                                      // the GEMM's +0-initialised accumulator
#pragma unroll
                    for (int c = 0; c < KIN; ++c) a = __builtin_fmaf(xv[r][c], wc[c][e], a);
                }
                if (has_b_in) a = a + bc[e];
                if (act0) a = ACT::fwd(a);
                h[r][j][e] = a;
            }
    }
}

// one square layer in place: diag_apply_kernel's row poison, r * wbar_diag + 0, + bias, the activation (hr).  lw: the layer's
// diagonal, lb: its bias (LDS).  MASK (the ReLU backward): bit (r C + j) 4 + e of *mask = the fused ReLU's gradient passes
// there, as whvi_diag_apply_bwd recomputes it -- from the layer's input BEFORE the poison: !(relu_(h * w (+ b)) <= 0), NaN passes
template <int LOG2D, int R, bool MASK = false, typename ACT = MlpRelu>
__device__ __forceinline__ void mlp_square_layer(float (&h)[R][MlpGeom<LOG2D>::C][4], const float *lw, const float *lb,
                                                 uint32_t col, bool hb, bool hr, uint32_t *mask = nullptr)
{
    static_assert(!MASK || !ACT::SMOOTH, "masks are the ReLU backward's");
    using Gm = MlpGeom<LOG2D>;
    constexpr int L = Gm::L, C = Gm::C;
    typedef float f4 __attribute__((ext_vector_type(4)));
    bool bad = false;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < C; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) bad |= !__builtin_isfinite(h[r][j][e]);
    const bool poison = __builtin_amdgcn_ballot_w64(bad) != 0;
    if (poison) {
        if constexpr (MASK) {
            uint32_t mk = 0;
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const f4 wc = reinterpret_cast<const f4 *>(lw)[col + j * L];
                const f4 bc = reinterpret_cast<const f4 *>(lb)[col + j * L];
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float z = h[r][j][e] * wc[e];
                        if (hb) z = z + bc[e];
                        if (!(relu_(z) <= 0.0f)) mk |= 1u << ((r * C + j) * 4 + e);
                    }
            }
            *mask = mk;
        }
        mlp_poison_rows<L, R, C>(h);
    }
    uint32_t mk = 0;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const uint32_t q = col + j * L;
        const f4 wc = reinterpret_cast<const f4 *>(lw)[q];
        const f4 bc = reinterpret_cast<const f4 *>(lb)[q];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = h[r][j][e] * wc[e] + 0.0f;               // the one non-zero product + the accumulator's +0
                if (hb) v = v + bc[e];
                if constexpr (MASK) {
                    if (!(relu_(v) <= 0.0f)) mk |= 1u << ((r * C + j) * 4 + e);
                }
                if (hr) v = ACT::fwd(v);
                h[r][j][e] = v;
            }
    }
    if constexpr (MASK) {
        if (!poison) *mask = mk;
    }
}

// y[s, b] for b in the block's slab.  x : (B, KIN); w_in : (S, D, KIN) (KIN = 4 / 8) or (S, D) (KIN = 1); s1, s2, b_mid :
// (n_mid, D); u : (n_mid, 1 + S, D) (mean row first, whvi_diag_apply's WHVI_DIAG_MEAN_PLUS layout); w_out : (S, D).
// act bit 0: ACT behind the first layer, bit 1 + m: behind square layer m.  mid_bias bit m: square layer m has a bias.
// TWIN: mlp_apply_kernel below repeats this body statement for statement with ACT = MlpRelu (see there why); a change to
// one -- tails, geometry, the row dot -- must be made in both.
template <int LOG2D, int KIN, typename ACT>
__device__ __forceinline__ void
mlp_apply_block(float *__restrict__ y, const float *__restrict__ x, const float *__restrict__ w_in,
                const float *__restrict__ b_in, const float *__restrict__ s1, const float *__restrict__ s2,
                const float *__restrict__ u, const float *__restrict__ b_mid, const float *__restrict__ w_out,
                const float *__restrict__ b_out, uint32_t S, uint32_t B, uint32_t n_mid, uint32_t mid_bias, uint32_t act,
                uint32_t slab_rows, uint32_t n_slabs)
{
    using Gm = MlpGeom<LOG2D>;
    constexpr int D = Gm::D, L = Gm::L, C = Gm::C, R = Gm::R, RPI = Gm::RPI;
    typedef float f4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float mlp_lds[];
    float *lw1 = mlp_lds;                    // [c][n]: KIN rows of D
    float *lbi = lw1 + KIN * D;              // b_in
    float *lmid = lbi + D;                   // square layer m: diagonal at 2 m D, bias at (2 m + 1) D
    float *lwo = lmid + 2 * n_mid * D;       // w_out

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t b0 = slab * slab_rows, b1 = b0 + slab_rows < B ? b0 + slab_rows : B;

    mlp_stage_operands<LOG2D, KIN>(mlp_lds, s, w_in, b_in, s1, s2, u, b_mid, w_out, S, n_mid, mid_bias);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t grp = (uint32_t)lane / L, col = (uint32_t)lane % L;      // the lane's row group and first chunk
    const bool has_b_in = b_in != nullptr;
    const float bo = b_out != nullptr ? b_out[0] : 0.0f;
    float *ys = y + (size_t)s * B;
    for (uint32_t rb = b0 + wave * RPI; rb < b1; rb += 4 * RPI) {
        // D >= 512 with a smooth activation: re-read the operands from LDS on every iteration instead of letting them be
        // hoisted into registers (as mlp_apply_bwd_block does): tanhf's temporaries on top took K = 8, D = 1024 past 256
        if constexpr (C >= 4) asm volatile("" ::: "memory");
        const uint32_t r0 = rb + grp * R;                 // rows r0 .. r0 + R - 1 (past b1: a valid row's operands, never stored)
        float h[R][C][4];
        {   // ---- first layer
            float xv[R][KIN];
            mlp_load_x<KIN, R>(xv, x, r0, b1);
            mlp_first_layer<LOG2D, KIN, R, ACT>(h, xv, lw1, lbi, col, has_b_in, (act & 1u) != 0);
        }
        // ---- square layers
        for (uint32_t m = 0; m < n_mid; ++m)
            mlp_square_layer<LOG2D, R, false, ACT>(h, lmid + 2 * m * D, lmid + (2 * m + 1) * D, col, (mid_bias >> m) & 1u,
                                                   (act >> (m + 1)) & 1u);
        // ---- transposed column layer: row_dot_kernel's partials, order and butterfly
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
            if (col == (uint32_t)r) outv = v;              // every lane of the group holds the sum: lane r keeps row r's
        }
        if (b_out != nullptr) outv = outv + bo;
        if (col < (uint32_t)R && r0 + col < b1) ys[r0 + col] = outv;      // R neighbouring floats per lane group
    }
}

// The ReLU pass.  It keeps a body of its own rather than calling mlp_apply_block, whose code is the same statement for statement:
// behind a call the inliner optimises the body before the kernel, and the ReLU kernels' code would change.  TWIN of
// mlp_apply_block: a change to one must be made in both (tests/test_mlp_smooth_gpu.py checks both against float64).
template <typename T, int LOG2D, int KIN>      // (T = float; named so that whvi_last_kernel prints the real symbol)
__global__ void __launch_bounds__(256)
mlp_apply_kernel(float *__restrict__ y, const float *__restrict__ x, const float *__restrict__ w_in, const float *__restrict__ b_in,
                 const float *__restrict__ s1, const float *__restrict__ s2, const float *__restrict__ u,
                 const float *__restrict__ b_mid, const float *__restrict__ w_out, const float *__restrict__ b_out, uint32_t S,
                 uint32_t B, uint32_t n_mid, uint32_t mid_bias, uint32_t relu, uint32_t slab_rows, uint32_t n_slabs)
{
    using Gm = MlpGeom<LOG2D>;
    constexpr int D = Gm::D, L = Gm::L, C = Gm::C, R = Gm::R, RPI = Gm::RPI;
    typedef float f4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float mlp_lds[];
    float *lw1 = mlp_lds;                    // [c][n]: KIN rows of D
    float *lbi = lw1 + KIN * D;              // b_in
    float *lmid = lbi + D;                   // square layer m: diagonal at 2 m D, bias at (2 m + 1) D
    float *lwo = lmid + 2 * n_mid * D;       // w_out

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t b0 = slab * slab_rows, b1 = b0 + slab_rows < B ? b0 + slab_rows : B;

    mlp_stage_operands<LOG2D, KIN>(mlp_lds, s, w_in, b_in, s1, s2, u, b_mid, w_out, S, n_mid, mid_bias);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t grp = (uint32_t)lane / L, col = (uint32_t)lane % L;      // the lane's row group and first chunk
    const bool has_b_in = b_in != nullptr;
    const float bo = b_out != nullptr ? b_out[0] : 0.0f;
    float *ys = y + (size_t)s * B;
    for (uint32_t rb = b0 + wave * RPI; rb < b1; rb += 4 * RPI) {
        const uint32_t r0 = rb + grp * R;                 // rows r0 .. r0 + R - 1 (past b1: a valid row's operands, never stored)
        float h[R][C][4];
        {   // ---- first layer
            float xv[R][KIN];
            mlp_load_x<KIN, R>(xv, x, r0, b1);
            mlp_first_layer<LOG2D, KIN, R>(h, xv, lw1, lbi, col, has_b_in, (relu & 1u) != 0);
        }
        // ---- square layers
        for (uint32_t m = 0; m < n_mid; ++m)
            mlp_square_layer<LOG2D, R>(h, lmid + 2 * m * D, lmid + (2 * m + 1) * D, col, (mid_bias >> m) & 1u, (relu >> (m + 1)) & 1u);
        // ---- transposed column layer: row_dot_kernel's partials, order and butterfly
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
            if (col == (uint32_t)r) outv = v;              // every lane of the group holds the sum: lane r keeps row r's
        }
        if (b_out != nullptr) outv = outv + bo;
        if (col < (uint32_t)R && r0 + col < b1) ys[r0 + col] = outv;      // R neighbouring floats per lane group
    }
}

// the same pass with a smooth activation, ACT = WHVI_MLP_ACT_SIGMOID / _TANH, at the boundaries of `act`
template <typename T, int LOG2D, int KIN, int ACT>
__global__ void __launch_bounds__(256)
mlp_smooth_apply_kernel(float *__restrict__ y, const float *__restrict__ x, const float *__restrict__ w_in,
                        const float *__restrict__ b_in, const float *__restrict__ s1, const float *__restrict__ s2,
                        const float *__restrict__ u, const float *__restrict__ b_mid, const float *__restrict__ w_out,
                        const float *__restrict__ b_out, uint32_t S, uint32_t B, uint32_t n_mid, uint32_t mid_bias, uint32_t act,
                        uint32_t slab_rows, uint32_t n_slabs)
{
    static_assert(MlpAct<ACT>::type::SMOOTH, "the ReLU pass is mlp_apply_kernel");
    mlp_apply_block<LOG2D, KIN, typename MlpAct<ACT>::type>(y, x, w_in, b_in, s1, s2, u, b_mid, w_out, b_out, S, B, n_mid,
                                                             mid_bias, act, slab_rows, n_slabs);
}

// The launch of one call, from mlp_apply_check
struct MlpLaunch {
    dim3 grid;
    size_t lds;
    uint32_t slab_rows, n_slabs;
};

// Every argument check of whvi_mlp_apply_f32 / whvi_mlp_apply_act_f32, before any launch; `bits` (named `bits_name` in the
// message) are the activation bits.  WHVI_OK with ln.grid.x = 0: nothing to launch.
inline int mlp_apply_check(MlpLaunch &ln, const void *y, const void *x, int32_t first, const void *w_in, const void *b_in,
                           int32_t n_mid, const void *s1, const void *s2, const void *u, const void *b_mid, int32_t mid_bias,
                           const void *w_out, const void *b_out, int64_t S, int64_t B, int32_t log2d, int32_t bits,
                           const char *bits_name)
{
    ln.grid = dim3(0);
    if (S < 0 || B < 0) return fail(WHVI_ERR_ARG, "whvi_mlp_apply: negative size%s", "");
    if (first != WHVI_MLP_FIRST_COLUMN && first != WHVI_MLP_FIRST_K4 && first != WHVI_MLP_FIRST_K8)
        return fail(WHVI_ERR_ARG, "whvi_mlp_apply: unknown first-layer kind%s %lld", "", first);
    if (n_mid < 1 || n_mid > MLP_MAX_MID)
        return fail(WHVI_ERR_SIZE, "whvi_mlp_apply: n_mid%s = %lld square layers (1 .. 4 only)", "", n_mid);
    if (log2d < 6 || log2d > 11) return fail(WHVI_ERR_SIZE, "whvi_mlp_apply: log2(D)%s = %lld is outside [6, 11]", "", log2d);
    if (!mlp_supported(first, n_mid, log2d))
        return fail(WHVI_ERR_SIZE, "whvi_mlp_apply: the operands of one sample%s need %lld B of LDS (64 KiB at most)", "",
                    mlp_lds_bytes(first, n_mid, log2d));
    if (bits & ~((1 << (n_mid + 1)) - 1)) return fail(WHVI_ERR_ARG, "whvi_mlp_apply: unknown %s bits 0x%llx", bits_name, bits);
    if (mid_bias & ~((1 << n_mid) - 1)) return fail(WHVI_ERR_ARG, "whvi_mlp_apply: unknown mid_bias bits%s 0x%llx", "", mid_bias);
    const int64_t rows = S * B;
    if (rows == 0) return WHVI_OK;
    if (rows >= ((int64_t)1 << 32)) return fail(WHVI_ERR_SIZE, "whvi_mlp_apply: rows are indexed with 32 bits%s", "");
    if (!y || !x || !w_in || !s1 || !s2 || !u || !w_out || (mid_bias != 0 && !b_mid))
        return fail(WHVI_ERR_ARG, "whvi_mlp_apply: null pointer%s", "");
    if (((uintptr_t)y | (uintptr_t)x | (uintptr_t)w_in | (uintptr_t)b_in | (uintptr_t)s1 | (uintptr_t)s2 | (uintptr_t)u |
         (uintptr_t)b_mid | (uintptr_t)w_out | (uintptr_t)b_out) & 15)
        return fail(WHVI_ERR_ALIGN, "whvi_mlp_apply: a pointer%s is not 16-byte aligned", "");
    {
        const int64_t D = (int64_t)1 << log2d, kin = first;
        const struct { const void *p; int64_t n; } in[] = {
            {x, B * kin}, {w_in, S * D * kin}, {b_in, D}, {s1, n_mid * D}, {s2, n_mid * D}, {u, n_mid * (S + 1) * D},
            {b_mid, n_mid * D}, {w_out, S * D}, {b_out, 1}};
        const char *yp = (const char *)y, *ye = yp + rows * 4;
        for (const auto &t : in) {
            const char *p = (const char *)t.p;
            if (p != nullptr && p < ye && yp < p + t.n * 4) return fail(WHVI_ERR_OVERLAP, "whvi_mlp_apply: y overlaps an input%s", "");
        }
    }
    // slabs: about four blocks per CU over all samples, every wave of a block with at least one row group
    int64_t n_slabs = (4 * (int64_t)num_cu() + S - 1) / S;
    const int64_t min_rows = 4 * 64;                      // >= 4 waves x the widest row group (D = 64: 32 rows)
    const int64_t most = (B + min_rows - 1) / min_rows;
    if (n_slabs > most) n_slabs = most;
    if (n_slabs < 1) n_slabs = 1;
    const int64_t slab_rows = (B + n_slabs - 1) / n_slabs;
    n_slabs = (B + slab_rows - 1) / slab_rows;
    if (n_slabs * S >= ((int64_t)1 << 31)) return fail(WHVI_ERR_SIZE, "whvi_mlp_apply: too many blocks%s", "");
    ln.lds = (size_t)mlp_lds_bytes(first, n_mid, log2d);
    ln.grid = dim3((unsigned)(n_slabs * S));
    ln.slab_rows = (uint32_t)slab_rows;
    ln.n_slabs = (uint32_t)n_slabs;
    return WHVI_OK;
}

}  // namespace whvi
