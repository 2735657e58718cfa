#pragma once
// whvi_amd/csrc/fused_stacked_layer_bwd.hpp -- backward of the rectangular fastfood layer WITH its epilogue
// (fused_stacked_fwd.hpp: bias, the neighbouring ReLUs, the narrowing to n_cols) in ONE launch plus a tiny finishing launch:
// fused_stacked_bwd.hpp's launch with the two masks, the zero padding and the bias sum folded in, so that no masked or padded
// copy of grad_y, no relu(x) and no unmasked grad_x exists in memory.  ABI: include/whvi_hip.h
// (whvi_fused_shs_stacked_layer_bwd_f32).
//
// Per row, for j = 0 .. J - 1 (col = j D + n):
//     xin   = relu_in ? relu_(x) : x                      (diag_apply.hpp's relu_: NaN passes)
//     g_j[n] = 0                          for col >= n_cols   (those 16-byte chunks of grad_y and y are not read)
//            = relu_out ? (y[col] <= 0 ? +0 : gy[col]) : gy[col]   elsewhere  (a select: aten.threshold_backward)
//     grad_bias[col] += g_j[n]                            (BIAS; plain adds in the lane's tile order)
//     fused_shs_stacked_bwd_kernel's chain on (xin, g_j), unchanged, the zero chunks included
// and grad_x = relu_in ? (xin <= 0 ? +0 : gx) : gx is stored once per tile.  grad_x and the 3 J parameter gradients are, bit
// for bit, whvi_fused_shs_stacked_bwd_f32 on the masked, zero-padded g and on relu(x), followed by the mask on grad_x.
//
// Geometry, tile body, transforms, pinned sums, in-block reduction and slot order: fused_shs_stacked_bwd_kernel's.  Differences:
//   * grad_y and y have a row pitch of their own (ld floats, a runtime argument) and n_cols <= J D columns; only the last
//     segment can hold chunks past n_cols ((J - 1) D < n_cols).
//   * segment j of grad_y (and of y) is requested in front of the segment's FIRST transform and masked when it has arrived,
//     behind that transform: y's chunks are then live where t1 is not yet, and the registers in flight across the second
//     transform are the sibling's.
//   * BIAS: J D / 64 * 4 more pinned sums per lane (4 J for rows shorter than 256).  They go through the LDS in a SECOND pass,
//     after the 3 J D sums have left it, so the dynamic LDS stays 12 D J bytes; the slot grows to (3 + BIAS) D J floats,
//     [j][a | b | c][D] followed by [j][bias][D].
// No atomics, no allocation, no synchronisation: two calls give the same bits.
#include "dispatch.hpp"
#include "diag_apply.hpp"
#include "fused_bwd.hpp"

namespace whvi {

constexpr int FUSED_STACKED_LAYER_BWD_MIN_LOG2D = 6, FUSED_STACKED_LAYER_BWD_MAX_LOG2D = 11, FUSED_STACKED_LAYER_BWD_MAX_BLOCKS = 4;
constexpr uint32_t LAYER_BWD_OPT_RELU_IN = 1u, LAYER_BWD_OPT_RELU_OUT = 2u;
// fused_stacked_bwd_supported's rule, with and without a bias: the LDS holds the J triples only (48 KiB at most), and every
// (log2d, J, bias) of the rule builds without scratch
inline bool fused_stacked_layer_bwd_supported(int log2d, int64_t n_blocks, bool /*has_bias*/)
{
    if (log2d < FUSED_STACKED_LAYER_BWD_MIN_LOG2D || log2d > FUSED_STACKED_LAYER_BWD_MAX_LOG2D) return false;
    if (n_blocks < 2 || n_blocks > FUSED_STACKED_LAYER_BWD_MAX_BLOCKS) return false;
    return log2d <= 10 || n_blocks == 2;
}
// floats of one block's slot: J triples of grad_a, grad_b, grad_c partials, then J rows of grad_bias partials
inline int64_t fused_stacked_layer_bwd_part_floats(int log2d, int64_t n_blocks, bool has_bias)
{
    return n_blocks * ((int64_t)(has_bias ? 4 : 3) << log2d);
}

// acc = acc + g in the accumulation half of the register file (fused_bwd_acc's pinning; a plain add, no multiply)
__device__ __forceinline__ void fused_layer_bwd_add(float &acc, float g)
{
    float t;
    asm("v_accvgpr_read_b32 %0, %1" : "=v"(t) : "a"(acc));
    t = t + g;
    asm("v_accvgpr_write_b32 %0, %1" : "=a"(acc) : "v"(t));
}

// a pinned sum read where it is used (volatile: not hoisted out of the wave-order loop, where all sums would be live at once)
__device__ __forceinline__ float fused_layer_bwd_read(const float &acc)
{
    float t;
    asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(t) : "a"(acc));
    return t;
}

// part : (n_samples * n_slabs) slots of (3 + BIAS) D J floats.  gx (n_samples * stride, D) or NULL; gy, y (n_samples * stride,
// n_cols) at a row pitch of ldq chunks (y is read only with LAYER_BWD_OPT_RELU_OUT); ncq = n_cols / 4; x, a, b, c, x_shared as
// in fused_shs_stacked_bwd_kernel.  NT: gy and y are read and gx written with the non-temporal policy.
template <typename T, int LOG2D, int K, int J, bool BIAS, bool NT>
__global__ void __launch_bounds__(256)
fused_shs_stacked_layer_bwd_kernel(float *__restrict__ part, u32x4 *__restrict__ gx, const u32x4 *__restrict__ gy,
                                   const u32x4 *__restrict__ y, const u32x4 *__restrict__ x, const float *__restrict__ a,
                                   const float *__restrict__ b, const float *__restrict__ c, uint32_t n_samples, uint32_t stride,
                                   uint32_t slab_rows, uint32_t n_slabs, uint32_t x_shared, uint32_t ncq, uint32_t ldq, uint32_t opts)
{
    using E = Elem<T>;
    constexpr int VEC = E::VEC;
    static_assert(std::is_same<T, float>::value && VEC == 4, "float32 storage");
    static_assert(J >= 2 && J <= FUSED_STACKED_LAYER_BWD_MAX_BLOCKS, "J = 1 and J > 4 stay composed");
    constexpr int D = 1 << LOG2D, SH = LOG2D - 2;          // SH = log2(chunks per row)
    constexpr uint32_t CPR = 1u << SH;
    constexpr bool WIDE = SH >= 6;                          // a row fills at least one chunk per lane
    constexpr int NC = WIDE ? (int)CPR / 64 : 1;            // column chunks per lane
    constexpr uint32_t RPT = (uint32_t)(K * 64) >> SH;      // rows per tile
    constexpr bool KEEP_X = K * VEC <= 16;                  // the x tile stays in registers (D = 2048 reads it again: L2)
    constexpr int NB = BIAS ? J : 1;                        // rows of bias sums
    static_assert(K * 64 >= (int)CPR && K % NC == 0, "a tile holds whole rows");
    static_assert(K == fused_bwd_k(LOG2D, VEC), "the tile of fused_bwd_geom");
    typedef float f4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float fused_stacked_layer_bwd_lds[];

    const bool relu_in = (opts & LAYER_BWD_OPT_RELU_IN) != 0, relu_out = (opts & LAYER_BWD_OPT_RELU_OUT) != 0;
    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t r_begin = slab * slab_rows;
    const uint32_t r_end = (uint64_t)r_begin + slab_rows < stride ? r_begin + slab_rows : stride;
    constexpr uint32_t QUADS = (uint32_t)D / 4;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        f4 *const la = reinterpret_cast<f4 *>(fused_stacked_layer_bwd_lds + (size_t)3 * j * D);
        const f4 *const ga = reinterpret_cast<const f4 *>(a + ((size_t)j << LOG2D));
        const f4 *const gb = reinterpret_cast<const f4 *>(b + (((size_t)j * n_samples + s) << LOG2D));
        const f4 *const gc = reinterpret_cast<const f4 *>(c + ((size_t)j << LOG2D));
        for (uint32_t i = threadIdx.x; i < QUADS; i += 256) {
            la[i] = ga[i];
            la[QUADS + i] = gb[i];
            la[2 * QUADS + i] = gc[i];
        }
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // chunk k of the lane: its column chunk and its row within the tile (fused_shs_kernel's layout, chunk k * 64 + lane)
    auto colq = [&](int k) __attribute__((always_inline)) -> uint32_t {
        if constexpr (WIDE) return (uint32_t)(k % NC) * 64u + (uint32_t)lane;
        else return (uint32_t)lane & (CPR - 1);
    };
    auto row_in = [&](int k) __attribute__((always_inline)) -> uint32_t {
        if constexpr (WIDE) return (uint32_t)(k / NC);                        // wave-uniform
        else return (uint32_t)(k * 64 + lane) >> SH;
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
    // One tile: rows rt .. rt + RPT - 1, fused_shs_stacked_bwd_kernel's one clamped body (rows past the slab's end are
    // duplicates of its last row: computed, never summed or stored).
    auto tile = [&](uint32_t rt) __attribute__((always_inline)) {
        constexpr bool TAIL = RPT > 1;
        auto row_ok = [&](int k) __attribute__((always_inline)) -> bool { return !TAIL || rt + row_in(k) < r_end; };
        auto row_rd = [&](int k) __attribute__((always_inline)) -> uint32_t {
            if constexpr (!TAIL) return row_in(k);
            else return row_ok(k) ? row_in(k) : r_end - 1 - rt;
        };
        // chunk k of the lane sits at rel(k) chunks from the tile's (wave-uniform) base in a (rows, D) tensor, at rel_y(k) in
        // the rows of grad_y and y (pitch ldq < 2^30 chunks, at most 16 rows per tile)
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
        // segment j: fused_shs_stacked_bwd_kernel's segment on (xin, g_j, a_j, b_js, c_j)
        auto seg = [&](auto jc) __attribute__((always_inline)) {
            constexpr int j = decltype(jc)::value;
            constexpr bool LAST = j == J - 1;
            const f4 *const la = reinterpret_cast<const f4 *>(fused_stacked_layer_bwd_lds + (size_t)3 * j * D);
            const f4 *const lb = la + QUADS, *const lc = lb + QUADS;
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
                    const u32x4 one = {0x3f800000u, 0x3f800000u, 0x3f800000u, 0x3f800000u};     // (1.0f: passes)
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
                const f4 cv = lc[colq(k)];
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
                const f4 bv = lb[colq(k)];
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
                const f4 av = la[colq(k)];
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
                const f4 bv = lb[colq(k)];
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (row_ok(k)) fused_bwd_acc(acc_b[j][k % NC][e], r[k][e], t1[k][e]);
                    r[k][e] = bv[e] * r[k][e];
                }
            }
            fused_bwd_fwht<LOG2D, K, false>(r, lane);
            phase_fence();
            // ---- grad_c[j] += w xin;  gx (+)= c_j w, and behind the last segment the mask of the activation in FRONT
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float xv[VEC];
                if constexpr (KEEP_X) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) xv[e] = xk[k][e];
                } else {
                    unpack_x(pre[k], xv);
                }
                const f4 cv = lc[colq(k)];
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
        u32x4 *const gxt = gx + ((sample_row0 + rt) << SH);
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (gx != nullptr && row_ok(k)) st16<NT>(gxt + rel(k), E::pack(gxa[k]));
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
    float *const red = fused_stacked_layer_bwd_lds;
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

// ---- host side
struct FusedStackedLayerBwdArgs {
    void *grad_x, *grad_bias, *work;
    const void *grad_y, *y, *x, *a, *b, *c;
    int64_t n_blocks, n_samples, sample_stride, n_cols, ld;
    int32_t log2d;
    uint32_t opts;
    bool x_shared, nt;
    FusedBwdGeom geom;
};

template <typename T, int L, int J, bool BIAS>
inline void fused_stacked_layer_bwd_launch_one(const FusedStackedLayerBwdArgs &r, hipStream_t st)
{
    constexpr int K = fused_bwd_k(L, Elem<T>::VEC);
    const dim3 grid((unsigned)(r.n_samples * r.geom.n_slabs));
    const size_t lds = (size_t)J * fused_bwd_part_floats(L) * sizeof(float);
    note_launch<T>("fused_shs_stacked_layer_bwd_kernel", L, K, J, BIAS, r.nt);
#define WHVI_FUSED_STACKED_LAYER_BWD(NT)                                                                                \
    hipLaunchKernelGGL((fused_shs_stacked_layer_bwd_kernel<T, L, K, J, BIAS, NT>), grid, dim3(256), lds, st, (float *)r.work, \
                       (u32x4 *)r.grad_x, (const u32x4 *)r.grad_y, (const u32x4 *)r.y, (const u32x4 *)r.x, (const float *)r.a, \
                       (const float *)r.b, (const float *)r.c, (uint32_t)r.n_samples, (uint32_t)r.sample_stride,          \
                       (uint32_t)r.geom.slab_rows, (uint32_t)r.geom.n_slabs, r.x_shared ? 1u : 0u, (uint32_t)(r.n_cols / 4), \
                       (uint32_t)(r.ld / 4), r.opts)
    if (r.nt) WHVI_FUSED_STACKED_LAYER_BWD(true);
    else WHVI_FUSED_STACKED_LAYER_BWD(false);
#undef WHVI_FUSED_STACKED_LAYER_BWD
}

}  // namespace whvi
