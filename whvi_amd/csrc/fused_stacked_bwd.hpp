#pragma once
// whvi_amd/csrc/fused_stacked_bwd.hpp -- backward of the rectangular fastfood layer (fused_stacked_fwd.hpp: J square operators on the
// same rows, their outputs side by side) in ONE launch plus a tiny finishing launch: grad_x and the 3 J parameter gradients for
// all Monte-Carlo samples from grad_y (rows of J D) and x (rows of D), without a copy of a segment of grad_y, a per-block grad_x
// or a running sum in memory.  ABI: include/whvi_hip.h (whvi_fused_shs_stacked_bwd_f32).
//
// Per row, for j = 0 .. J - 1, fused_bwd.hpp's chain on segment j (gy_j = grad_y[r, j D : (j + 1) D]):
//     t1 = H(c_j x)
//     u  = H(b_js t1)                 grad_a[j]    += gy_j u
//     v  = H(a_j gy_j)                grad_b[j, s] += v t1
//     w  = H(b_js v)                  grad_c[j]    += w x
//     gx = c_0 w_0   (j = 0),         gx = gx + c_j w_j   (j > 0: the product and the add are separate roundings)
// and grad_x = gx is packed and stored once per tile, after the last j.  The operand bits, the transforms (fused_bwd_fwht), the
// fused multiply-adds (fused_bwd_acc), the tile-to-wave assignment and the block order are fused_shs_bwd_kernel's, so block j's
// three parameter gradients are, bit for bit, whvi_fused_shs_bwd_f32 on the contiguous copy of segment j, and grad_x is the
// per-block launches' grad_x added in ascending j.
//
// Geometry: fused_shs_bwd_kernel's, unchanged.  A block of four waves owns (sample s, a slab of that sample's rows) --
// fused_bwd_geom -- stages the J triples [a_j | b_{j,s} | c_j] in LDS as fused_shs_stacked_kernel does (12 D J bytes) and walks
// its slab one wave tile at a time (K = fused_bwd_k(LOG2D): one row from D = 1024 up, 1024 floats below; rows past the slab's
// end are clamped duplicates, computed and never summed or stored).  x's tile is loaded once per tile and kept in registers where
// fused_shs_bwd_kernel keeps it (D <= 1024); at D = 2048 it is read again through the caches.  Segment j of grad_y is requested
// in front of the second transform.
//
// Sums: J is a template argument, so the 3 J D / 64 per-lane sums (12 J for rows shorter than 256) are registers indexed by
// constants, pinned to the accumulation half of the register file (fused_bwd_acc).  After the slab: the same-column butterfly
// (rows shorter than 256), the four waves through the operands' LDS in wave order, one slot of 3 D J floats per block laid out
// [j][a | b | c][D].  fused_shs_stacked_bwd_finish_kernel adds the slots in ascending block order.  No atomics, no allocation,
// no synchronisation: two calls give the same bits.
#include "dispatch.hpp"
#include "fused_bwd.hpp"

namespace whvi {

constexpr int FUSED_STACKED_BWD_MIN_LOG2D = 6, FUSED_STACKED_BWD_MAX_LOG2D = 11, FUSED_STACKED_BWD_MAX_BLOCKS = 4;
// J = 1 is whvi_fused_shs_bwd_f32; the triples of J blocks fit 48 KiB of LDS (J <= 4 up to D = 1024, J = 2 at D = 2048)
inline bool fused_stacked_bwd_supported(int log2d, int64_t n_blocks)
{
    if (log2d < FUSED_STACKED_BWD_MIN_LOG2D || log2d > FUSED_STACKED_BWD_MAX_LOG2D) return false;
    if (n_blocks < 2 || n_blocks > FUSED_STACKED_BWD_MAX_BLOCKS) return false;
    return log2d <= 10 || n_blocks == 2;
}
// floats of one block's slot: J triples of grad_a, grad_b, grad_c partials
inline int64_t fused_stacked_bwd_part_floats(int log2d, int64_t n_blocks) { return n_blocks * fused_bwd_part_floats(log2d); }

// part : (n_samples * n_slabs) slots of 3 D J floats.  gx (n_samples * stride, D) or NULL; gy (n_samples * stride, J D); x
// (n_samples * stride, D), or (stride, D) with x_shared (row r of every sample reads x[r]).  a, c : (J, D); b : (J, n_samples, D).
// NT: gy is read and gx written with the non-temporal policy (streams larger than the Infinity Cache).
template <typename T, int LOG2D, int K, int J, bool NT>
__global__ void __launch_bounds__(256)
fused_shs_stacked_bwd_kernel(float *__restrict__ part, u32x4 *__restrict__ gx, const u32x4 *__restrict__ gy,
                             const u32x4 *__restrict__ x, const float *__restrict__ a, const float *__restrict__ b,
                             const float *__restrict__ c, uint32_t n_samples, uint32_t stride, uint32_t slab_rows, uint32_t n_slabs,
                             uint32_t x_shared)
{
    using E = Elem<T>;
    constexpr int VEC = E::VEC;
    static_assert(std::is_same<T, float>::value && VEC == 4, "float32 storage");
    static_assert(J >= 2 && J <= FUSED_STACKED_BWD_MAX_BLOCKS, "J = 1 is fused_shs_bwd_kernel");
    constexpr int D = 1 << LOG2D, SH = LOG2D - 2;          // SH = log2(chunks per row)
    constexpr uint32_t CPR = 1u << SH;
    constexpr bool WIDE = SH >= 6;                          // a row fills at least one chunk per lane
    constexpr int NC = WIDE ? (int)CPR / 64 : 1;            // column chunks per lane
    constexpr uint32_t RPT = (uint32_t)(K * 64) >> SH;      // rows per tile
    constexpr bool KEEP_X = K * VEC <= 16;                  // the x tile stays in registers (D = 2048 reads it again: L2)
    constexpr uint32_t PITCH = (uint32_t)J << SH;           // chunks of one row of grad_y
    static_assert(K * 64 >= (int)CPR && K % NC == 0, "a tile holds whole rows");
    static_assert(K == fused_bwd_k(LOG2D, VEC), "the tile of fused_bwd_geom");
    typedef float f4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float fused_stacked_bwd_lds[];

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t r_begin = slab * slab_rows;
    const uint32_t r_end = (uint64_t)r_begin + slab_rows < stride ? r_begin + slab_rows : stride;
    constexpr uint32_t QUADS = (uint32_t)D / 4;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        f4 *const la = reinterpret_cast<f4 *>(fused_stacked_bwd_lds + (size_t)3 * j * D);
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

    float acc_a[J][NC][VEC], acc_b[J][NC][VEC], acc_c[J][NC][VEC];
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int n = 0; n < NC; ++n)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc_a[j][n][e] = acc_b[j][n][e] = acc_c[j][n][e] = 0.0f;

    // between the phases of a tile: nothing is scheduled across, and the operands are read from LDS again where they are used
    auto phase_fence = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    // One tile: rows rt .. rt + RPT - 1.  Tiles of several rows (TAIL): rows past the slab's end are clamped duplicates --
    // computed (every lane takes part in the transforms), never summed or stored.  ONE body serves the full tiles and the
    // slab's last one (a few compares per chunk): a second, unclamped body costs a second set of the pinned sums' registers
    // (12 J .. 24 J) and 40 % more code, and a wave per SIMD at most (D, J) below 1024.
    auto tile = [&](uint32_t rt) __attribute__((always_inline)) {
        constexpr bool TAIL = RPT > 1;
        auto row_ok = [&](int k) __attribute__((always_inline)) -> bool { return !TAIL || rt + row_in(k) < r_end; };
        // the row of chunk k within the tile as it is read: its own, or the slab's last
        auto row_rd = [&](int k) __attribute__((always_inline)) -> uint32_t {
            if constexpr (!TAIL) return row_in(k);
            else return row_ok(k) ? row_in(k) : r_end - 1 - rt;
        };
        // chunk k of the lane sits at rel(k) chunks from the tile's (wave-uniform) base in a (rows, D) tensor, at rel_y(k) in
        // grad_y's rows of J D
        auto rel = [&](int k) __attribute__((always_inline)) -> uint32_t {
            if constexpr (!TAIL) return (uint32_t)(k * 64 + lane);
            else return (row_rd(k) << SH) + colq(k);
        };
        auto rel_y = [&](int k) __attribute__((always_inline)) -> uint32_t { return row_rd(k) * PITCH + colq(k); };
        const u32x4 *const xt = x + ((x_row0 + rt) << SH);
        const u32x4 *const gyt = gy + (sample_row0 + rt) * PITCH;
        float gxa[K][VEC], xk[KEEP_X ? K : 1][VEC];
        u32x4 pre[K];
        if constexpr (KEEP_X) {
#pragma unroll
            for (int k = 0; k < K; ++k) pre[k] = ld16<false>(xt + rel(k));
            phase_fence();
#pragma unroll
            for (int k = 0; k < K; ++k) E::unpack(pre[k], xk[k]);
        }
        // segment j: fused_shs_bwd_kernel's tile on (x, gy_j, a_j, b_js, c_j)
        auto seg = [&](auto jc) __attribute__((always_inline)) {
            constexpr int j = decltype(jc)::value;
            const f4 *const la = reinterpret_cast<const f4 *>(fused_stacked_bwd_lds + (size_t)3 * j * D);
            const f4 *const lb = la + QUADS, *const lc = lb + QUADS;
            float r[K][VEC], t1[K][VEC];
            // ---- t1 = H(c_j x)
            if constexpr (!KEEP_X) {
#pragma unroll
                for (int k = 0; k < K; ++k) pre[k] = ld16<false>(xt + rel(k));
                phase_fence();
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if constexpr (KEEP_X) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) r[k][e] = xk[k][e];
                } else {
                    E::unpack(pre[k], r[k]);
                }
                const f4 cv = lc[colq(k)];
#pragma unroll
                for (int e = 0; e < VEC; ++e) r[k][e] = cv[e] * r[k][e];
            }
            fused_bwd_fwht<LOG2D, K, true>(r, lane);
            // ---- u = H(b_js t1), with segment j of grad_y's tile requested in front of the transform
            phase_fence();
#pragma unroll
            for (int k = 0; k < K; ++k) pre[k] = ld16<NT>(gyt + ((uint32_t)j << SH) + rel_y(k));
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
            // ---- grad_a[j] += gy_j u;  v = H(a_j gy_j)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float gv[VEC];
                E::unpack(pre[k], gv);
                const f4 av = la[colq(k)];
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (row_ok(k)) fused_bwd_acc(acc_a[j][k % NC][e], gv[e], r[k][e]);
                    r[k][e] = av[e] * gv[e];
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
            // ---- grad_c[j] += w x;  gx (+)= c_j w
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float xv[VEC];
                if constexpr (KEEP_X) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) xv[e] = xk[k][e];
                } else {
                    E::unpack(pre[k], xv);
                }
                const f4 cv = lc[colq(k)];
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (row_ok(k)) fused_bwd_acc(acc_c[j][k % NC][e], r[k][e], xv[e]);
                    const float cw = cv[e] * r[k][e];
                    gxa[k][e] = j == 0 ? cw : gxa[k][e] + cw;
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
                }
    }
    __syncthreads();                                       // every wave is done with the operands: the LDS holds the sums now
    float *const red = fused_stacked_bwd_lds;
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
    float *p = part + (size_t)blockIdx.x * (3 * D * J);
    for (uint32_t i = threadIdx.x; i < 3u * D * J; i += 256) p[i] = red[i];
}

// ---- host side
struct FusedStackedBwdArgs {
    void *grad_x, *work;
    const void *grad_y, *x, *a, *b, *c;
    int64_t n_blocks, n_samples, sample_stride;
    int32_t log2d;
    bool x_shared, nt;
    FusedBwdGeom geom;
};

template <typename T, int L, int J>
inline void fused_stacked_bwd_launch_one(const FusedStackedBwdArgs &r, hipStream_t st)
{
    constexpr int K = fused_bwd_k(L, Elem<T>::VEC);
    const dim3 grid((unsigned)(r.n_samples * r.geom.n_slabs));
    const size_t lds = (size_t)J * fused_bwd_part_floats(L) * sizeof(float);
    note_launch<T>("fused_shs_stacked_bwd_kernel", L, K, J, r.nt);
#define WHVI_FUSED_STACKED_BWD(NT)                                                                                      \
    hipLaunchKernelGGL((fused_shs_stacked_bwd_kernel<T, L, K, J, NT>), grid, dim3(256), lds, st, (float *)r.work,         \
                       (u32x4 *)r.grad_x, (const u32x4 *)r.grad_y, (const u32x4 *)r.x, (const float *)r.a, (const float *)r.b, \
                       (const float *)r.c, (uint32_t)r.n_samples, (uint32_t)r.sample_stride, (uint32_t)r.geom.slab_rows,  \
                       (uint32_t)r.geom.n_slabs, r.x_shared ? 1u : 0u)
    if (r.nt) WHVI_FUSED_STACKED_BWD(true);
    else WHVI_FUSED_STACKED_BWD(false);
#undef WHVI_FUSED_STACKED_BWD
}

}  // namespace whvi
