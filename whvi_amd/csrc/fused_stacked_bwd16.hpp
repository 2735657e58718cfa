#pragma once
// whvi_amd/csrc/fused_stacked_bwd16.hpp -- backward of the rectangular fastfood layer on 16-bit activation streams in ONE launch
// plus a tiny finishing launch: fused_shs_stacked_bwd_kernel (fused_stacked_bwd.hpp: J square operators on the same rows, the
// J-segment structure, the pinned sums, one tile body, the slot layout) with fused_shs_bwd_kernel<__half | __hip_bfloat16>'s
// 8-element chunks (fused_bwd.hpp: the split LDS layout, KEEP_X, pack-then-store).  ABI: include/whvi_hip.h
// (whvi_fused_shs_stacked_bwd_f16 / _bf16).
//
// Per row, for j = 0 .. J - 1, on the exactly-upcast x and gy_j = grad_y[r, j D : (j + 1) D], all in float32:
//     t1 = H(c_j x)
//     u  = H(b_js t1)                 grad_a[j]    += gy_j u
//     v  = H(a_j gy_j)                grad_b[j, s] += v t1
//     w  = H(b_js v)                  grad_c[j]    += w x
//     gx = c_0 w_0   (j = 0),         gx = gx + c_j w_j   (j > 0: the product and the add are separate roundings)
// gx stays float32 across the segments and is rounded to 16 bits ONCE, after the last j: the whole tile is packed into registers
// of its own and only then stored.  So grad_x is whvi_fused_shs_stacked_bwd_f32 on the exact upcasts, cast once -- not the
// per-block 16-bit launches' grad_x added in 16 bits (2 J - 1 roundings).  Block j's three parameter gradients are, bit for bit,
// whvi_fused_shs_bwd_f16 / _bf16 on the contiguous copy of segment j (the same operand bits, transforms, fused multiply-adds,
// tile-to-wave assignment and block order), and from D = 512 up (a row fills at least one chunk per lane) the float32 stacked
// launch's on the upcasts.
//
// Geometry: fused_bwd_geom, unchanged.  A block of four waves owns (sample s, a slab of that sample's rows), stages the J
// float32 triples [a_j | b_{j,s} | c_j] in LDS (12 D J bytes), each vector in fused16.hpp's split layout (the first halves of
// all chunks, then the second halves: both 16-byte reads of a chunk's eight factors are lane-contiguous), and walks its slab one
// wave tile at a time (K = fused_bwd_k(LOG2D, 8); rows past the slab's end are clamped duplicates, computed and never summed
// or stored).  x's tile stays in registers up to D = 1024; at D = 2048 it is read again through the caches.
//
// Sums: 3 J D / 64 per lane (24 J for rows shorter than 64 chunks, D < 512), pinned to the accumulation half of the register
// file (fused_bwd_acc).  After the slab: the same-column butterfly (D < 512), the four waves through the operands' LDS in wave
// order, one slot of 3 D J floats per block laid out [j][a | b | c][D]; fused_stacked_bwd16_finish_kernel adds the slots in
// ascending block order (fused_shs_stacked_bwd_finish_kernel's summation order).  No atomics, no allocation, no
// synchronisation: two calls give the same bits.
#include "dispatch.hpp"
#include "fused_bwd.hpp"
#include "fused_stacked_bwd.hpp"

namespace whvi {

// the float32 launch's range: the staged triples are float32 either way
inline bool fused_stacked_bwd16_supported(int log2d, int64_t n_blocks) { return fused_stacked_bwd_supported(log2d, n_blocks); }

// part : (n_samples * n_slabs) slots of 3 D J floats.  gx (n_samples * stride, D) 16-bit or NULL; gy (n_samples * stride, J D)
// 16-bit; x (n_samples * stride, D) 16-bit, or (stride, D) with x_shared.  a, c : (J, D) float32; b : (J, n_samples, D) float32.
// NT: gy is read and gx written with the non-temporal policy (streams larger than the Infinity Cache).
template <typename T, int LOG2D, int K, int J, bool NT>
__global__ void __launch_bounds__(256)
fused_stacked_bwd16_kernel(float *__restrict__ part, u32x4 *__restrict__ gx, const u32x4 *__restrict__ gy,
                           const u32x4 *__restrict__ x, const float *__restrict__ a, const float *__restrict__ b,
                           const float *__restrict__ c, uint32_t n_samples, uint32_t stride, uint32_t slab_rows, uint32_t n_slabs,
                           uint32_t x_shared)
{
    using E = Elem<T>;
    constexpr int VEC = E::VEC;
    static_assert(sizeof(T) == 2 && VEC == 8 && std::is_same<typename E::acc, float>::value, "16-bit storage, float32 arithmetic");
    static_assert(J >= 2 && J <= FUSED_STACKED_BWD_MAX_BLOCKS, "J = 1 is fused_shs_bwd_kernel");
    constexpr int D = 1 << LOG2D, SH = LOG2D - 3;           // SH = log2(chunks per row)
    constexpr uint32_t CPR = 1u << SH;
    constexpr bool WIDE = SH >= 6;                          // a row fills at least one chunk per lane
    constexpr int NC = WIDE ? (int)CPR / 64 : 1;            // column chunks per lane
    constexpr uint32_t RPT = (uint32_t)(K * 64) >> SH;      // rows per tile
    constexpr bool KEEP_X = K * VEC <= 16;                  // the x tile stays in registers (D = 2048 reads it again: L2)
    constexpr uint32_t PITCH = (uint32_t)J << SH;           // chunks of one row of grad_y
    static_assert(K * 64 >= (int)CPR && K % NC == 0, "a tile holds whole rows");
    static_assert(K == fused_bwd_k(LOG2D, VEC), "the tile of fused_bwd_geom");
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef FusedBwdFactors<VEC> factors_t;
    extern __shared__ __attribute__((aligned(16))) float fused_stacked_bwd16_lds[];

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t r_begin = slab * slab_rows;
    const uint32_t r_end = (uint64_t)r_begin + slab_rows < stride ? r_begin + slab_rows : stride;
    // piece i of a vector (16 bytes) goes to half (i & 1) of chunk i >> 1 in the split layout
    constexpr uint32_t QUADS = (uint32_t)D / 4;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        f4 *const la = reinterpret_cast<f4 *>(fused_stacked_bwd16_lds + (size_t)3 * j * D);
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
    // slab's last one, as in fused_shs_stacked_bwd_kernel: a second body costs a second set of the pinned sums' registers.
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
            const float *const la = fused_stacked_bwd16_lds + (size_t)3 * j * D;
            const float *const lb = la + D, *const lc = lb + D;
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
                const factors_t cv = factors(lc, k);
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
                const factors_t bv = factors(lb, k);
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
                const factors_t av = factors(la, k);
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
                const factors_t bv = factors(lb, k);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (row_ok(k)) fused_bwd_acc(acc_b[j][k % NC][e], r[k][e], t1[k][e]);
                    r[k][e] = bv[e] * r[k][e];
                }
            }
            fused_bwd_fwht<LOG2D, K, false>(r, lane);
            phase_fence();
            // ---- grad_c[j] += w x;  gx (+)= c_j w, in float32
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float xv[VEC];
                if constexpr (KEEP_X) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) xv[e] = xk[k][e];
                } else {
                    E::unpack(pre[k], xv);
                }
                const factors_t cv = factors(lc, k);
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
                }
    }
    __syncthreads();                                       // every wave is done with the operands: the LDS holds the sums now
    float *const red = fused_stacked_bwd16_lds;
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

// ---- host side: one checked call = the launch above plus the finishing launch.  The checks and the finishing kernel are
// compiled once (fused_stacked_bwd_f16.hip); each storage type's translation unit instantiates its own kernels through
// fused_stacked_bwd16_run<T>.

// Every argument check of whvi_fused_shs_stacked_bwd_f16 / _bf16, before any device call: fused_stacked_bwd_check's, in its
// order, the extents of x, grad_y and grad_x counted in 2-byte elements.  WHVI_OK with launch = false: nothing to launch.
int fused_stacked_bwd16_check(FusedStackedBwdArgs &r, bool &launch, void *grad_x, void *grad_a, void *grad_b, void *grad_c,
                              void *work, const void *grad_y, const void *x, const void *a, const void *b, const void *c, int64_t J,
                              int64_t S, int64_t stride, int32_t log2d, int32_t flags);
// fused_stacked_bwd16_finish_kernel on the slots of r's grid
int fused_stacked_bwd16_finish(const FusedStackedBwdArgs &r, void *grad_a, void *grad_b, void *grad_c, hipStream_t st);

template <typename T, int L, int J>
inline void fused_stacked_bwd16_launch_one(const FusedStackedBwdArgs &r, hipStream_t st)
{
    constexpr int K = fused_bwd_k(L, Elem<T>::VEC);
    const dim3 grid((unsigned)(r.n_samples * r.geom.n_slabs));
    const size_t lds = (size_t)J * fused_bwd_part_floats(L) * sizeof(float);
    note_launch<T>("fused_stacked_bwd16_kernel", L, K, J, r.nt);
#define WHVI_FUSED_STACKED_BWD16(NT)                                                                                    \
    hipLaunchKernelGGL((fused_stacked_bwd16_kernel<T, L, K, J, NT>), grid, dim3(256), lds, st, (float *)r.work,           \
                       (u32x4 *)r.grad_x, (const u32x4 *)r.grad_y, (const u32x4 *)r.x, (const float *)r.a, (const float *)r.b, \
                       (const float *)r.c, (uint32_t)r.n_samples, (uint32_t)r.sample_stride, (uint32_t)r.geom.slab_rows,  \
                       (uint32_t)r.geom.n_slabs, r.x_shared ? 1u : 0u)
    if (r.nt) WHVI_FUSED_STACKED_BWD16(true);
    else WHVI_FUSED_STACKED_BWD16(false);
#undef WHVI_FUSED_STACKED_BWD16
}

template <typename T, int L>
inline void fused_stacked_bwd16_launch(const FusedStackedBwdArgs &r, hipStream_t st)
{
    if constexpr (L <= 10) {
        switch (r.n_blocks) {
        case 2: fused_stacked_bwd16_launch_one<T, L, 2>(r, st); break;
        case 3: fused_stacked_bwd16_launch_one<T, L, 3>(r, st); break;
        default: fused_stacked_bwd16_launch_one<T, L, 4>(r, st); break;
        }
    } else {
        fused_stacked_bwd16_launch_one<T, L, 2>(r, st);
    }
}

template <typename T>
inline int fused_stacked_bwd16_run(void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *work, const void *grad_y,
                                   const void *x, const void *a, const void *b, const void *c, int64_t n_blocks, int64_t n_samples,
                                   int64_t sample_stride, int32_t log2d, int32_t flags, void *stream)
{
    FusedStackedBwdArgs r;
    bool launch = false;
    int rc = fused_stacked_bwd16_check(r, launch, grad_x, grad_a, grad_b, grad_c, work, grad_y, x, a, b, c, n_blocks, n_samples,
                                       sample_stride, log2d, flags);
    if (rc != WHVI_OK || !launch) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (log2d) {
    case 6: fused_stacked_bwd16_launch<T, 6>(r, st); break;
    case 7: fused_stacked_bwd16_launch<T, 7>(r, st); break;
    case 8: fused_stacked_bwd16_launch<T, 8>(r, st); break;
    case 9: fused_stacked_bwd16_launch<T, 9>(r, st); break;
    case 10: fused_stacked_bwd16_launch<T, 10>(r, st); break;
    default: fused_stacked_bwd16_launch<T, 11>(r, st); break;
    }
    rc = after_launch("fused_shs_stacked_bwd (16-bit)");
    if (rc != WHVI_OK) return rc;
    return fused_stacked_bwd16_finish(r, grad_a, grad_b, grad_c, st);
}

}  // namespace whvi
