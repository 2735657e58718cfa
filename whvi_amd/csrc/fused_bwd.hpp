#pragma once
// whvi_amd/csrc/fused_bwd.hpp -- backward of the fused pipeline y = a (.) H(b_s (.) H(c (.) x)) (fused_shs_kernel, axis = COL,
// shared a / c, per-sample b) in ONE launch plus a tiny finishing launch: grad_x and the three parameter gradients for all
// Monte-Carlo samples from grad_y and x, without any saved or materialised intermediate.  ABI: include/whvi_hip.h
// (whvi_fused_shs_bwd_f32).
//
// Per row, last to first -- FastfoodFunction.backward's composition, what mlp_fastfood_apply_bwd.hpp runs per square layer:
//     t1 = H(c x)                     (recomputed, kept in registers)
//     u  = H(b_s t1)                  grad_a    += grad_y u
//     v  = H(a grad_y)                grad_b[s] += v t1
//     w  = H(b_s v)                   grad_c    += w x
//     grad_x = c w
// Every multiply of the chain is its own rounding and the butterflies are fwht_tile with the forward's template arguments
// and sign sequence (0 -> SIGN_MID -> 0), so grad_x is, bit for bit, whvi_fused_shs_f32(grad_y, a := c, b, c := a) -- the
// launch that computes grad_x when no parameter wants a gradient.  t1 and v both carry the lane-sign convention SIGN_MID,
// which cancels in their product; u and w carry none.  The three sums are fused multiply-adds into per-lane registers.
//
// Ownership: rows are in the Module's layout, rows == n_samples * sample_stride with sample s at [s stride, (s + 1) stride).
// A block of four waves owns (sample s, a slab of that sample's rows), stages a, b_s and c in LDS (12 D bytes) and walks the
// slab one wave tile at a time.  A tile is K chunks of 16 bytes per lane in fused_shs_kernel's layout (chunk k * 64 + lane):
// one row for D >= 1024, 1024 / D rows below.  Butterflies are per row, so the tile size changes no value.
//
// Sums (as mlp_fastfood_apply_bwd.hpp): each lane keeps the sums of its columns over its rows in registers (3 D / 64 floats,
// 12 for rows shorter than 256); lanes that share a column (rows shorter than 256: the tile puts several rows side by side
// in a wave) combine by a butterfly; the four waves add through the LDS that held the operands, in wave order; the block
// writes one partial per field to its slot of the workspace.  fused_shs_bwd_finish_kernel adds the slots in ascending block
// order -- the blocks of sample s for grad_b[s], all blocks for grad_a and grad_c.  No atomics, no allocation: two calls give
// the same bits.
#include "kernels.hpp"

namespace whvi {

constexpr int FUSED_BWD_MIN_LOG2D = 6, FUSED_BWD_MAX_LOG2D = 12;
inline bool fused_bwd_supported(int log2d) { return log2d >= FUSED_BWD_MIN_LOG2D && log2d <= FUSED_BWD_MAX_LOG2D; }

// chunks per lane of one wave tile: one row from D = 1024 up (4, 8, 16), 1024 floats (2 .. 16 rows) below
constexpr int fused_bwd_k(int log2d) { return log2d >= 10 ? 1 << (log2d - 8) : 4; }
constexpr int64_t fused_bwd_tile_rows(int log2d) { return ((int64_t)fused_bwd_k(log2d) * 256) >> log2d; }

// The grid of one call, a function of the arguments alone (the workspace query and the launch share it; no device query):
// blocks = n_samples * n_slabs, aimed at 1024 in all (512 for D = 4096, whose blocks run one per CU: two rounds on a 256-CU
// part; two to four blocks per CU are resident below), every slab a multiple of the tile's rows and long enough to give
// each of the block's four waves a tile -- small launches get few blocks.
struct FusedBwdGeom { int64_t n_slabs, slab_rows; };
inline FusedBwdGeom fused_bwd_geom(int64_t n_samples, int64_t sample_stride, int log2d)
{
    const int64_t rpt = fused_bwd_tile_rows(log2d), target = log2d >= 12 ? 512 : 1024;
    int64_t n = (target + n_samples - 1) / n_samples;
    const int64_t most = (sample_stride + 4 * rpt - 1) / (4 * rpt);
    if (n > most) n = most;
    if (n < 1) n = 1;
    int64_t slab = (sample_stride + n - 1) / n;
    slab = (slab + rpt - 1) / rpt * rpt;
    FusedBwdGeom g;
    g.slab_rows = slab;
    g.n_slabs = (sample_stride + slab - 1) / slab;
    return g;
}
// floats of one block's slot: grad_a, grad_b, grad_c partials, D each
constexpr int64_t fused_bwd_part_floats(int log2d) { return (int64_t)3 << log2d; }

// the two transforms of the pipeline as fused_shs_kernel issues them: FIRST from sign mask 0 (leaves SIGN_MID), the second
// from SIGN_MID (leaves 0)
template <int LOG2D, int K, bool FIRST>
__device__ __forceinline__ void fused_bwd_fwht(float (&r)[K][4], int lane)
{
    constexpr bool SIGNED = WHVI_FUSED_SIGNED != 0;
    constexpr int SIGN_MID = SIGNED ? fwht_sign_out<4, LOG2D>(0) : 0;
    static_assert(!SIGNED || fwht_sign_out<4, LOG2D>(SIGN_MID) == 0, "two transforms restore the sign convention");
    fwht_tile<float, 4, K, LOG2D, POLICY_DPP, WHVI_FUSED_PKMASK, SIGNED, FIRST ? 0 : SIGN_MID>(r, lane);
}

// acc = fma(p, q, acc), with the sum pinned to the accumulation half of the wave's register file -- read out, updated, written
// back.  The 3 D / 64 sums then never compete with the tile, t1 and the butterflies' temporaries for the arithmetic
// registers: left to the allocator, D = 4096 spills 164 registers to scratch and D = 2048 needs 335 registers (one wave per
// SIMD); pinned, they take 245 + 192 and 124 + 96 (two waves per SIMD), and D <= 1024 gains a wave per SIMD as well.
__device__ __forceinline__ void fused_bwd_acc(float &acc, float p, float q)
{
    float t;
    asm("v_accvgpr_read_b32 %0, %1" : "=v"(t) : "a"(acc));
    t = __builtin_fmaf(p, q, t);
    asm("v_accvgpr_write_b32 %0, %1" : "=a"(acc) : "v"(t));
}

// part : (n_samples * n_slabs) slots of 3 D floats.  gx (n_samples * stride, D) or NULL; gy likewise; x the same, or
// (stride, D) with x_shared (WHVI_FUSED_SRC_SHARED: row r of every sample reads x[r]).  a, c : (D); b : (n_samples, D).
// NT: gy is read and gx written with the non-temporal policy (streams larger than the Infinity Cache).
template <typename T, int LOG2D, int K, bool NT>        // (T = float; named so that whvi_last_kernel prints the real symbol)
__global__ void __launch_bounds__(256)
fused_shs_bwd_kernel(float *__restrict__ part, u32x4 *__restrict__ gx, const u32x4 *__restrict__ gy, const u32x4 *__restrict__ x,
                     const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ c, uint32_t stride,
                     uint32_t slab_rows, uint32_t n_slabs, uint32_t x_shared)
{
    static_assert(std::is_same<T, float>::value, "float32 only");
    constexpr int D = 1 << LOG2D, SH = LOG2D - 2;           // SH = log2(chunks per row)
    constexpr uint32_t CPR = 1u << SH;
    constexpr bool WIDE = SH >= 6;                          // a row fills at least one chunk per lane
    constexpr int NC = WIDE ? (int)CPR / 64 : 1;            // column chunks per lane
    constexpr uint32_t RPT = (uint32_t)(K * 64) >> SH;      // rows per tile
    constexpr bool KEEP_X = K <= 4;                         // the x tile stays in registers for grad_c (D >= 2048 reads it again: L2)
    static_assert(K * 64 >= (int)CPR && K % NC == 0, "a tile holds whole rows");
    typedef float f4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float fused_bwd_lds[];
    float *const la = fused_bwd_lds, *const lb = la + D, *const lc = lb + D;

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t r_begin = slab * slab_rows, r_end = r_begin + slab_rows < stride ? r_begin + slab_rows : stride;
    for (uint32_t i = threadIdx.x; i < CPR; i += 256) {
        reinterpret_cast<f4 *>(la)[i] = reinterpret_cast<const f4 *>(a)[i];
        reinterpret_cast<f4 *>(lb)[i] = reinterpret_cast<const f4 *>(b + ((size_t)s << LOG2D))[i];
        reinterpret_cast<f4 *>(lc)[i] = reinterpret_cast<const f4 *>(c)[i];
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

    float acc_a[NC][4], acc_b[NC][4], acc_c[NC][4];
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc_a[j][e] = acc_b[j][e] = acc_c[j][e] = 0.0f;

    // between the phases of a tile: nothing is scheduled across, and the operands are read from LDS again where they are used
    // (a value of b or c kept from its first use to its second would stay live across two transforms)
    auto phase_fence = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    // One tile: rows rt .. rt + RPT - 1.  TAIL (tiles of several rows only): rows past the slab's end are clamped duplicates --
    // computed (every lane takes part in the transforms), never summed or stored.
    auto tile = [&](uint32_t rt, auto tail) __attribute__((always_inline)) {
        constexpr bool TAIL = decltype(tail)::value != 0;
        // chunk k of the lane sits at rel(k) chunks from the tile's (wave-uniform) base in a (rows, D) tensor
        auto row_ok = [&](int k) __attribute__((always_inline)) -> bool { return !TAIL || rt + row_in(k) < r_end; };
        auto rel = [&](int k) __attribute__((always_inline)) -> uint32_t {
            if constexpr (!TAIL) return (uint32_t)(k * 64 + lane);
            else return ((row_ok(k) ? row_in(k) : r_end - 1 - rt) << SH) + colq(k);
        };
        const u32x4 *const xt = x + ((x_row0 + rt) << SH);
        const u32x4 *const gyt = gy + ((sample_row0 + rt) << SH);
        float r[K][4], t1[K][4], xk[KEEP_X ? K : 1][4];
        u32x4 pre[K];
        // ---- t1 = H(c x)
#pragma unroll
        for (int k = 0; k < K; ++k) pre[k] = ld16<false>(xt + rel(k));
        phase_fence();
#pragma unroll
        for (int k = 0; k < K; ++k) {
            Elem<float>::unpack(pre[k], r[k]);
            const f4 cv = reinterpret_cast<const f4 *>(lc)[colq(k)];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (KEEP_X) xk[k][e] = r[k][e];
                r[k][e] = cv[e] * r[k][e];
            }
        }
        fused_bwd_fwht<LOG2D, K, true>(r, lane);
        // ---- u = H(b_s t1), with grad_y's tile requested in front of the transform
        phase_fence();
#pragma unroll
        for (int k = 0; k < K; ++k) pre[k] = ld16<NT>(gyt + rel(k));
        phase_fence();
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const f4 bv = reinterpret_cast<const f4 *>(lb)[colq(k)];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                t1[k][e] = r[k][e];
                r[k][e] = bv[e] * r[k][e];
            }
        }
        fused_bwd_fwht<LOG2D, K, false>(r, lane);
        phase_fence();
        // ---- grad_a += grad_y u;  v = H(a grad_y)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float gv[4];
            Elem<float>::unpack(pre[k], gv);
            const f4 av = reinterpret_cast<const f4 *>(la)[colq(k)];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (row_ok(k)) fused_bwd_acc(acc_a[k % NC][e], gv[e], r[k][e]);
                r[k][e] = av[e] * gv[e];
            }
        }
        fused_bwd_fwht<LOG2D, K, true>(r, lane);
        // ---- grad_b[s] += v t1;  w = H(b_s v), with x's tile requested again in front of the transform where it was not kept
        phase_fence();
        if constexpr (!KEEP_X) {
#pragma unroll
            for (int k = 0; k < K; ++k) pre[k] = ld16<false>(xt + rel(k));
            phase_fence();
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const f4 bv = reinterpret_cast<const f4 *>(lb)[colq(k)];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (row_ok(k)) fused_bwd_acc(acc_b[k % NC][e], r[k][e], t1[k][e]);
                r[k][e] = bv[e] * r[k][e];
            }
        }
        fused_bwd_fwht<LOG2D, K, false>(r, lane);
        phase_fence();
        // ---- grad_c += w x;  grad_x = c w
        u32x4 *const gxt = gx + ((sample_row0 + rt) << SH);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float xv[4];
            if constexpr (KEEP_X) {
#pragma unroll
                for (int e = 0; e < 4; ++e) xv[e] = xk[k][e];
            } else {
                Elem<float>::unpack(pre[k], xv);
            }
            const f4 cv = reinterpret_cast<const f4 *>(lc)[colq(k)];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (row_ok(k)) fused_bwd_acc(acc_c[k % NC][e], r[k][e], xv[e]);
                r[k][e] = cv[e] * r[k][e];
            }
            if (gx != nullptr && row_ok(k)) st16<NT>(gxt + rel(k), Elem<float>::pack(r[k]));
        }
    };
    // the loop bound is wave-uniform: every lane of the wave takes part in the DPP / permlane stages of the transforms
    for (uint32_t rt = r_begin + (uint32_t)wave * RPT; rt < r_end; rt += 4 * RPT) {
        asm volatile("" ::: "memory");          // re-read the operands from LDS on every tile rather than hoisting 3 D / 64 registers
        if constexpr (RPT > 1) {
            if (rt + RPT <= r_end) tile(rt, IC<0>{});
            else tile(rt, IC<1>{});
        } else {
            tile(rt, IC<0>{});
        }
    }

    // ---- the block's sums: lanes that share a column by a butterfly, then the waves through LDS in wave order
    if constexpr (!WIDE) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int m = (int)CPR; m < 64; m <<= 1) {
                acc_a[0][e] = acc_a[0][e] + __shfl_xor(acc_a[0][e], m, 64);
                acc_b[0][e] = acc_b[0][e] + __shfl_xor(acc_b[0][e], m, 64);
                acc_c[0][e] = acc_c[0][e] + __shfl_xor(acc_c[0][e], m, 64);
            }
    }
    __syncthreads();                                       // every wave is done with the operands: the LDS holds the sums now
    float *const red = fused_bwd_lds;
    for (int w = 0; w < 4; ++w) {
        if (wave == w && (WIDE || (uint32_t)lane < CPR)) {
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const uint32_t q = WIDE ? (uint32_t)j * 64u + (uint32_t)lane : (uint32_t)lane;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t n = 4 * q + e;
                    red[n] = w == 0 ? acc_a[j][e] : red[n] + acc_a[j][e];
                    red[D + n] = w == 0 ? acc_b[j][e] : red[D + n] + acc_b[j][e];
                    red[2 * D + n] = w == 0 ? acc_c[j][e] : red[2 * D + n] + acc_c[j][e];
                }
            }
        }
        __syncthreads();
    }
    float *p = part + (size_t)blockIdx.x * (3 * D);
    for (uint32_t i = threadIdx.x; i < 3u * D; i += 256) p[i] = red[i];
}

// the backward launch for one row length (defined in fused_bwd_f32.hip, where the instantiations are compiled)
struct FusedBwdArgs {
    void *grad_x, *work;
    const void *grad_y, *x, *a, *b, *c;
    int64_t n_samples, sample_stride;
    int32_t log2d;
    bool x_shared, nt;
    FusedBwdGeom geom;
};

}  // namespace whvi
