#pragma once
// whvi_amd/csrc/fused_stacked_layer_bwd16.hpp -- backward of the rectangular fastfood layer WITH its epilogue on 16-bit
// activation streams in ONE launch plus a tiny finishing launch: fused_stacked_bwd16_kernel (fused_stacked_bwd16.hpp: the
// 8-element chunks, the split LDS layout, KEEP_X, pack-then-store) with fused_shs_stacked_layer_bwd_kernel's folds
// (fused_stacked_layer_bwd.hpp: the masks of both ReLUs, the zero padding past n_cols, the bias sum), so that no masked or
// padded copy of grad_y, no relu(x) and no unmasked grad_x exists in memory.  ABI: include/whvi_hip.h
// (whvi_fused_shs_stacked_layer_bwd_f16 / _bf16).
//
// Per row, for j = 0 .. J - 1 (col = j D + n), on the exact upcasts, all in float32:
//     xin    = relu_in ? relu_(x) : x                     (diag_apply.hpp's relu_: NaN passes)
//     g_j[n] = 0                          for col >= n_cols   (those 16-byte chunks of grad_y and y are not read)
//            = relu_out ? (y[col] <= 0 ? +0 : gy[col]) : gy[col]   elsewhere  (a select: aten.threshold_backward)
//     grad_bias[col] += g_j[n]                            (BIAS; plain float32 adds in the lane's tile order)
//     fused_stacked_bwd16_kernel's chain on (xin, g_j), unchanged, the zero chunks included
// gx stays float32 across the segments and is rounded to 16 bits ONCE; grad_x = relu_in ? (xin <= 0 ? +0 : pack(gx)) : pack(gx)
// is stored once per tile (the select commutes with the rounding: it is applied to the float32 value in front of the pack).
// grad_x and the 3 J parameter gradients are, bit for bit, whvi_fused_shs_stacked_bwd_f16 / _bf16 on the masked, zero-padded
// 16-bit g and on relu(x), followed by the 16-bit mask on grad_x: the masked values are exact in 16 bits.
//
// Geometry, tile body, transforms, pinned sums, in-block reduction and slot order: fused_stacked_bwd16_kernel's.  Differences
// (fused_shs_stacked_layer_bwd_kernel's, on 8-element chunks):
//   * grad_y and y have a row pitch of their own (ld elements, a runtime argument, a multiple of 8) and n_cols <= J D columns
//     (a multiple of 8); only the last segment can hold chunks past n_cols ((J - 1) D < n_cols).
//   * segment j of grad_y (and of y) is requested in front of the segment's FIRST transform and masked when it has arrived,
//     behind that transform.
//   * BIAS: J D / 64 more pinned sums per lane (8 J for rows shorter than 512).  They go through the LDS in a SECOND pass,
//     after the 3 J D sums have left it, so the dynamic LDS stays 12 D J bytes; the slot grows to (3 + BIAS) D J floats,
//     [j][a | b | c][D] followed by [j][bias][D] -- the float32 launch's slot, workspace and grid.
// No atomics, no allocation, no synchronisation: two calls give the same bits.
#include "dispatch.hpp"
#include "diag_apply.hpp"
#include "fused_bwd.hpp"
#include "fused_stacked_layer_bwd.hpp"

namespace whvi {

// the float32 launch's range: the staged triples and the pinned sums are float32 either way, and every (log2d, J, bias) of the
// rule builds without scratch
inline bool fused_layer_bwd16_supported(int log2d, int64_t n_blocks, bool has_bias)
{
    return fused_stacked_layer_bwd_supported(log2d, n_blocks, has_bias);
}

// part : (n_samples * n_slabs) slots of (3 + BIAS) D J floats.  gx (n_samples * stride, D) 16-bit or NULL; gy, y (n_samples *
// stride, n_cols) 16-bit at a row pitch of ldq chunks (y is read only with LAYER_BWD_OPT_RELU_OUT); ncq = n_cols / 8; x
// (n_samples * stride, D) 16-bit, or (stride, D) with x_shared.  a, c : (J, D) float32; b : (J, n_samples, D) float32.
// NT: gy and y are read and gx written with the non-temporal policy.
template <typename T, int LOG2D, int K, int J, bool BIAS, bool NT>
__global__ void __launch_bounds__(256)
fused_layer_bwd16_kernel(float *__restrict__ part, u32x4 *__restrict__ gx, const u32x4 *__restrict__ gy,
                         const u32x4 *__restrict__ y, const u32x4 *__restrict__ x, const float *__restrict__ a,
                         const float *__restrict__ b, const float *__restrict__ c, uint32_t n_samples, uint32_t stride,
                         uint32_t slab_rows, uint32_t n_slabs, uint32_t x_shared, uint32_t ncq, uint32_t ldq, uint32_t opts)
{
    using E = Elem<T>;
    constexpr int VEC = E::VEC;
    static_assert(sizeof(T) == 2 && VEC == 8 && std::is_same<typename E::acc, float>::value, "16-bit storage, float32 arithmetic");
    static_assert(J >= 2 && J <= FUSED_STACKED_LAYER_BWD_MAX_BLOCKS, "J = 1 and J > 4 stay composed");
    constexpr int D = 1 << LOG2D, SH = LOG2D - 3;           // SH = log2(chunks per row)
    constexpr uint32_t CPR = 1u << SH;
    constexpr bool WIDE = SH >= 6;                          // a row fills at least one chunk per lane
    constexpr int NC = WIDE ? (int)CPR / 64 : 1;            // column chunks per lane
    constexpr uint32_t RPT = (uint32_t)(K * 64) >> SH;      // rows per tile
    constexpr bool KEEP_X = K * VEC <= 16;                  // the x tile stays in registers (D = 2048 reads it again: L2)
    constexpr int NB = BIAS ? J : 1;                        // rows of bias sums
    static_assert(K * 64 >= (int)CPR && K % NC == 0, "a tile holds whole rows");
    static_assert(K == fused_bwd_k(LOG2D, VEC), "the tile of fused_bwd_geom");
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef FusedBwdFactors<VEC> factors_t;
    extern __shared__ __attribute__((aligned(16))) float fused_layer_bwd16_lds[];

    const bool relu_in = (opts & LAYER_BWD_OPT_RELU_IN) != 0, relu_out = (opts & LAYER_BWD_OPT_RELU_OUT) != 0;
    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t r_begin = slab * slab_rows;
    const uint32_t r_end = (uint64_t)r_begin + slab_rows < stride ? r_begin + slab_rows : stride;
    // piece i of a vector (16 bytes) goes to half (i & 1) of chunk i >> 1 in the split layout
    constexpr uint32_t QUADS = (uint32_t)D / 4;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        f4 *const la = reinterpret_cast<f4 *>(fused_layer_bwd16_lds + (size_t)3 * j * D);
        const f4 *const ga = reinterpret_cast<const f4 *>(a + ((size_t)j << LOG2D));
        const f4 *const gb = reinterpret_cast<const f4 *>(b + (((size_t)j * n_samples + s) << LOG2D));
        const f4 *const gc = reinterpret_cast<const f4 *>(c + ((size_t)j << LOG2D));
        for (uint32_t i = threadIdx.x; i < QUADS; i += 256) {
            const uint32_t q = (i & 1) * (QUADS / 2) + (i >> 1);
            la[q] = ga[i];
            la[QUADS + q] = gb[i];
            la[2 * QUADS + q] = gc[i];
        }
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // chunk k of the lane: its column chunk and its row within the tile (fused_shs16_kernel's layout, chunk k * 64 + lane)
    auto colq = [&](int k) __attribute__((always_inline)) -> uint32_t {
        if constexpr (WIDE) return (uint32_t)(k % NC) * 64u + (uint32_t)lane;
        else return (uint32_t)lane & (CPR - 1);
    };
    auto row_in = [&](int k) __attribute__((always_inline)) -> uint32_t {
        if constexpr (WIDE) return (uint32_t)(k / NC);                        // wave-uniform
        else return (uint32_t)(k * 64 + lane) >> SH;
    };
    // the factors of the lane's chunk k of a staged vector
    auto factors = [&](const float *v, int k) __attribute__((always_inline)) -> factors_t {
        factors_t f;
        f.q[0] = reinterpret_cast<const f4 *>(v)[colq(k)];
        f.q[1] = reinterpret_cast<const f4 *>(v + D / 2)[colq(k)];
        return f;
    };
    const size_t sample_row0 = (size_t)s * stride;
    const size_t x_row0 = x_shared ? 0 : sample_row0;

    float acc_a[J][NC][VEC], acc_b[J][NC][VEC], acc_c[J][NC][VEC], acc_h[NB][NC][VEC];
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int n = 0; n < NC; ++n)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc_a[j][n][e] = acc_b[j][n][e] = acc_c[j][n][e] = 0.0f;
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int n = 0; n < NC; ++n)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc_h[j][n][e] = 0.0f;

    // between the phases of a tile: nothing is scheduled across, and the operands are read from LDS again where they are used
    auto phase_fence = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    // One tile: rows rt .. rt + RPT - 1, fused_stacked_bwd16_kernel's one clamped body (rows past the slab's end are
    // duplicates of its last row: computed, never summed or stored).
    auto tile = [&](uint32_t rt) __attribute__((always_inline)) {
        constexpr bool TAIL = RPT > 1;
        auto row_ok = [&](int k) __attribute__((always_inline)) -> bool { return !TAIL || rt + row_in(k) < r_end; };
        auto row_rd = [&](int k) __attribute__((always_inline)) -> uint32_t {
            if constexpr (!TAIL) return row_in(k);
            else return row_ok(k) ? row_in(k) : r_end - 1 - rt;
        };
        // chunk k of the lane sits at rel(k) chunks from the tile's (wave-uniform) base in a (rows, D) tensor, at rel_y(k) in
        // the rows of grad_y and y (pitch ldq < 2^29 chunks, at most 16 rows per tile)
        auto rel = [&](int k) __attribute__((always_inline)) -> uint32_t {
            if constexpr (!TAIL) return (uint32_t)(k * 64 + lane);
            else return (row_rd(k) << SH) + colq(k);
        };
        auto rel_y = [&](int k) __attribute__((always_inline)) -> size_t { return (size_t)row_rd(k) * ldq + colq(k); };
        const u32x4 *const xt = x + ((x_row0 + rt) << SH);
        const u32x4 *const gyt = gy + (sample_row0 + rt) * ldq;
        float gxa[K][VEC], xk[KEEP_X ? K : 1][VEC];
        u32x4 pre[K];
        // the activation in FRONT of the layer, on the unpacked tile
        auto unpack_x = [&](const u32x4 &raw, float (&o)[VEC]) __attribute__((always_inline)) {
            E::unpack(raw, o);
            if (relu_in) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) o[e] = relu_(o[e]);
            }
        };
        if constexpr (KEEP_X) {
#pragma unroll
            for (int k = 0; k < K; ++k) pre[k] = ld16<false>(xt + rel(k));
            phase_fence();
#pragma unroll
            for (int k = 0; k < K; ++k) unpack_x(pre[k], xk[k]);
        }
        // segment j: fused_stacked_bwd16_kernel's segment on (xin, g_j, a_j, b_js, c_j)
        auto seg = [&](auto jc) __attribute__((always_inline)) {
            constexpr int j = decltype(jc)::value;
            constexpr bool LAST = j == J - 1;
            const float *const la = fused_layer_bwd16_lds + (size_t)3 * j * D;
            const float *const lb = la + D, *const lc = lb + D;
            // chunk k lies inside n_cols (only the last segment reaches past it)
            auto in_cols = [&](int k) __attribute__((always_inline)) -> bool {
                return !LAST || ((uint32_t)j << SH) + colq(k) < ncq;
            };
            float r[K][VEC], t1[K][VEC], g[K][VEC];
            u32x4 gq[K], yq[K];
            // ---- t1 = H(c_j xin), with segment j of grad_y's (and y's) tile requested in front of the transform
            if constexpr (!KEEP_X) {
#pragma unroll
                for (int k = 0; k < K; ++k) pre[k] = ld16<false>(xt + rel(k));
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const u32x4 z = {0u, 0u, 0u, 0u};
                gq[k] = z;
                if (in_cols(k)) gq[k] = ld16<NT>(gyt + ((uint32_t)j << SH) + rel_y(k));
            }
            if (relu_out) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    // (two 1.0 of the storage type: passes)
                    constexpr uint32_t ONE2 = std::is_same<T, __half>::value ? 0x3c003c00u : 0x3f803f80u;
                    const u32x4 one = {ONE2, ONE2, ONE2, ONE2};
                    yq[k] = one;
                    if (in_cols(k)) yq[k] = ld16<NT>(y + (sample_row0 + rt) * ldq + ((uint32_t)j << SH) + rel_y(k));
                }
            }
            phase_fence();
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if constexpr (KEEP_X) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) r[k][e] = xk[k][e];
                } else {
                    unpack_x(pre[k], r[k]);
                }
                const factors_t cv = factors(lc, k);
#pragma unroll
                for (int e = 0; e < VEC; ++e) r[k][e] = cv[e] * r[k][e];
            }
            fused_bwd_fwht<LOG2D, K, true>(r, lane);
            // ---- g_j: the mask of the activation BEHIND the layer (a select); grad_bias[j] += g_j;  u = H(b_js t1)
            phase_fence();
#pragma unroll
            for (int k = 0; k < K; ++k) {
                E::unpack(gq[k], g[k]);
                if (relu_out) {
                    float yv[VEC];
                    E::unpack(yq[k], yv);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) g[k][e] = yv[e] <= 0.0f ? 0.0f : g[k][e];
                }
                if constexpr (BIAS) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e)
                        if (row_ok(k)) fused_layer_bwd_add(acc_h[BIAS ? j : 0][k % NC][e], g[k][e]);
                }
            }
            phase_fence();
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const factors_t bv = factors(lb, k);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    t1[k][e] = r[k][e];
                    r[k][e] = bv[e] * r[k][e];
                }
            }
            fused_bwd_fwht<LOG2D, K, false>(r, lane);
            phase_fence();
            // ---- grad_a[j] += g_j u;  v = H(a_j g_j)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const factors_t av = factors(la, k);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (row_ok(k)) fused_bwd_acc(acc_a[j][k % NC][e], g[k][e], r[k][e]);
                    r[k][e] = av[e] * g[k][e];
                }
            }
            fused_bwd_fwht<LOG2D, K, true>(r, lane);
            // ---- grad_b[j, s] += v t1;  w = H(b_js v), with x's tile requested again in front of the transform where it was
            // not kept
            phase_fence();
            if constexpr (!KEEP_X) {
#pragma unroll
                for (int k = 0; k < K; ++k) pre[k] = ld16<false>(xt + rel(k));
                phase_fence();
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const factors_t bv = factors(lb, k);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (row_ok(k)) fused_bwd_acc(acc_b[j][k % NC][e], r[k][e], t1[k][e]);
                    r[k][e] = bv[e] * r[k][e];
                }
            }
            fused_bwd_fwht<LOG2D, K, false>(r, lane);
            phase_fence();
            // ---- grad_c[j] += w xin;  gx (+)= c_j w in float32, and behind the last segment the mask of the activation in
            // FRONT (on the float32 value: the select commutes with the one rounding)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float xv[VEC];
                if constexpr (KEEP_X) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) xv[e] = xk[k][e];
                } else {
                    unpack_x(pre[k], xv);
                }
                const factors_t cv = factors(lc, k);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (row_ok(k)) fused_bwd_acc(acc_c[j][k % NC][e], r[k][e], xv[e]);
                    const float cw = cv[e] * r[k][e];
                    float v = j == 0 ? cw : gxa[k][e] + cw;
                    if (LAST && relu_in) v = xv[e] <= 0.0f ? 0.0f : v;
                    gxa[k][e] = v;
                }
            }
            phase_fence();
        };
        seg(IC<0>{});
        seg(IC<1>{});
        if constexpr (J > 2) seg(IC<2>{});
        if constexpr (J > 3) seg(IC<3>{});
        // the one rounding to 16 bits: the whole tile is packed first, into registers of its own, and only then stored -- no pack
        // writes a register that a store issued just before it still reads (fused16.hpp)
        u32x4 *const gxt = gx + ((sample_row0 + rt) << SH);
        u32x4 packed[K];
#pragma unroll
        for (int k = 0; k < K; ++k) packed[k] = E::pack(gxa[k]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (gx != nullptr && row_ok(k)) st16<NT>(gxt + rel(k), packed[k]);
    };
    // the loop bound is wave-uniform: every lane of the wave takes part in the DPP / permlane stages of the transforms
    for (uint32_t rt = r_begin + (uint32_t)wave * RPT; rt < r_end; rt += 4 * RPT) {
        asm volatile("" ::: "memory");          // re-read the operands from LDS on every tile rather than hoisting them
        tile(rt);
    }

    // ---- the block's sums: lanes that share a column by a butterfly, then the waves through LDS in wave order
    if constexpr (!WIDE) {
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < VEC; ++e)
#pragma unroll
                for (int m = (int)CPR; m < 64; m <<= 1) {
                    acc_a[j][0][e] = acc_a[j][0][e] + __shfl_xor(acc_a[j][0][e], m, 64);
                    acc_b[j][0][e] = acc_b[j][0][e] + __shfl_xor(acc_b[j][0][e], m, 64);
                    acc_c[j][0][e] = acc_c[j][0][e] + __shfl_xor(acc_c[j][0][e], m, 64);
                    if constexpr (BIAS) acc_h[BIAS ? j : 0][0][e] = acc_h[BIAS ? j : 0][0][e] + __shfl_xor(acc_h[BIAS ? j : 0][0][e], m, 64);
                }
    }
    __syncthreads();                                       // every wave is done with the operands: the LDS holds the sums now
    float *const red = fused_layer_bwd16_lds;
    for (int w = 0; w < 4; ++w) {
        if (wave == w && (WIDE || (uint32_t)lane < CPR)) {
#pragma unroll
            for (int j = 0; j < J; ++j)
#pragma unroll
                for (int n = 0; n < NC; ++n) {
                    const uint32_t q = WIDE ? (uint32_t)n * 64u + (uint32_t)lane : (uint32_t)lane;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const uint32_t i = (uint32_t)(3 * j) * D + VEC * q + e;
                        red[i] = w == 0 ? acc_a[j][n][e] : red[i] + acc_a[j][n][e];
                        red[D + i] = w == 0 ? acc_b[j][n][e] : red[D + i] + acc_b[j][n][e];
                        red[2 * D + i] = w == 0 ? acc_c[j][n][e] : red[2 * D + i] + acc_c[j][n][e];
                    }
                }
        }
        __syncthreads();
    }
    constexpr uint32_t SLOT = (uint32_t)(BIAS ? 4 : 3) * D * J;
    float *p = part + (size_t)blockIdx.x * SLOT;
    for (uint32_t i = threadIdx.x; i < 3u * D * J; i += 256) p[i] = red[i];
    if constexpr (BIAS) {
        // the second pass: the bias sums through the first J D floats of the LDS, in wave order
        __syncthreads();
        for (int w = 0; w < 4; ++w) {
            if (wave == w && (WIDE || (uint32_t)lane < CPR)) {
#pragma unroll
                for (int j = 0; j < J; ++j)
#pragma unroll
                    for (int n = 0; n < NC; ++n) {
                        const uint32_t q = WIDE ? (uint32_t)n * 64u + (uint32_t)lane : (uint32_t)lane;
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            const uint32_t i = (uint32_t)j * D + VEC * q + e;
                            const float h = fused_layer_bwd_read(acc_h[BIAS ? j : 0][n][e]);
                            red[i] = w == 0 ? h : red[i] + h;
                        }
                    }
            }
            __syncthreads();
        }
        for (uint32_t i = threadIdx.x; i < (uint32_t)D * J; i += 256) p[3u * D * J + i] = red[i];
    }
}

// ---- host side: one checked call = the launch above plus the finishing launch.  The checks and the finishing kernel are
// compiled once (fused_stacked_layer_bwd_f16.hip); each storage type's translation unit instantiates its own kernels through
// fused_layer_bwd16_run<T>.

// Every argument check of whvi_fused_shs_stacked_layer_bwd_f16 / _bf16, before any device call: the float32 entry's, in its
// order and with its codes, the extents of x, grad_y, y and grad_x counted in 2-byte elements and n_cols, ld in multiples of 8.
// WHVI_OK with launch = false: nothing to launch.
int fused_layer_bwd16_check(FusedStackedLayerBwdArgs &r, bool &launch, void *grad_x, void *grad_a, void *grad_b, void *grad_c,
                            void *grad_bias, void *work, const void *grad_y, const void *y, const void *x, const void *a,
                            const void *b, const void *c, int64_t J, int64_t S, int64_t stride, int32_t log2d, int64_t n_cols,
                            int64_t ld, int32_t flags);
// fused_layer_bwd16_finish_kernel on the slots of r's grid
int fused_layer_bwd16_finish(const FusedStackedLayerBwdArgs &r, void *grad_a, void *grad_b, void *grad_c, hipStream_t st);

template <typename T, int L, int J, bool BIAS>
inline void fused_layer_bwd16_launch_one(const FusedStackedLayerBwdArgs &r, hipStream_t st)
{
    constexpr int K = fused_bwd_k(L, Elem<T>::VEC);
    const dim3 grid((unsigned)(r.n_samples * r.geom.n_slabs));
    const size_t lds = (size_t)J * fused_bwd_part_floats(L) * sizeof(float);
    note_launch<T>("fused_layer_bwd16_kernel", L, K, J, BIAS, r.nt);
#define WHVI_FUSED_LAYER_BWD16(NT)                                                                                      \
    hipLaunchKernelGGL((fused_layer_bwd16_kernel<T, L, K, J, BIAS, NT>), grid, dim3(256), lds, st, (float *)r.work,       \
                       (u32x4 *)r.grad_x, (const u32x4 *)r.grad_y, (const u32x4 *)r.y, (const u32x4 *)r.x, (const float *)r.a, \
                       (const float *)r.b, (const float *)r.c, (uint32_t)r.n_samples, (uint32_t)r.sample_stride,          \
                       (uint32_t)r.geom.slab_rows, (uint32_t)r.geom.n_slabs, r.x_shared ? 1u : 0u, (uint32_t)(r.n_cols / 8), \
                       (uint32_t)(r.ld / 8), r.opts)
    if (r.nt) WHVI_FUSED_LAYER_BWD16(true);
    else WHVI_FUSED_LAYER_BWD16(false);
#undef WHVI_FUSED_LAYER_BWD16
}

template <typename T, int L, bool BIAS>
inline void fused_layer_bwd16_launch(const FusedStackedLayerBwdArgs &r, hipStream_t st)
{
    if constexpr (L <= 10) {
        switch (r.n_blocks) {
        case 2: fused_layer_bwd16_launch_one<T, L, 2, BIAS>(r, st); break;
        case 3: fused_layer_bwd16_launch_one<T, L, 3, BIAS>(r, st); break;
        default: fused_layer_bwd16_launch_one<T, L, 4, BIAS>(r, st); break;
        }
    } else {
        fused_layer_bwd16_launch_one<T, L, 2, BIAS>(r, st);
    }
}

template <typename T, bool BIAS>
inline void fused_layer_bwd16_launch_l(const FusedStackedLayerBwdArgs &r, hipStream_t st)
{
    switch (r.log2d) {
    case 6: fused_layer_bwd16_launch<T, 6, BIAS>(r, st); break;
    case 7: fused_layer_bwd16_launch<T, 7, BIAS>(r, st); break;
    case 8: fused_layer_bwd16_launch<T, 8, BIAS>(r, st); break;
    case 9: fused_layer_bwd16_launch<T, 9, BIAS>(r, st); break;
    case 10: fused_layer_bwd16_launch<T, 10, BIAS>(r, st); break;
    default: fused_layer_bwd16_launch<T, 11, BIAS>(r, st); break;
    }
}

template <typename T>
inline int fused_layer_bwd16_run(void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *grad_bias, void *work,
                                 const void *grad_y, const void *y, const void *x, const void *a, const void *b, const void *c,
                                 int64_t n_blocks, int64_t n_samples, int64_t sample_stride, int32_t log2d, int64_t n_cols,
                                 int64_t ld, int32_t flags, void *stream)
{
    FusedStackedLayerBwdArgs r;
    bool launch = false;
    int rc = fused_layer_bwd16_check(r, launch, grad_x, grad_a, grad_b, grad_c, grad_bias, work, grad_y, y, x, a, b, c, n_blocks,
                                     n_samples, sample_stride, log2d, n_cols, ld, flags);
    if (rc != WHVI_OK || !launch) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (grad_bias != nullptr) fused_layer_bwd16_launch_l<T, true>(r, st);
    else fused_layer_bwd16_launch_l<T, false>(r, st);
    rc = after_launch("fused_shs_stacked_layer_bwd (16-bit)");
    if (rc != WHVI_OK) return rc;
    return fused_layer_bwd16_finish(r, grad_a, grad_b, grad_c, st);
}

}  // namespace whvi
