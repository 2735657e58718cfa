#pragma once
// whvi_amd/csrc/fused_bwd.hpp -- backward of the fused pipeline y = a (.) H(b_s (.) H(c (.) x)) (fused_shs_kernel, axis = COL,
// shared a / c, per-sample b) in ONE launch plus a tiny finishing launch: grad_x and the three parameter gradients for all
// Monte-Carlo samples from grad_y and x, without any saved or materialised intermediate.  ABI: include/whvi_hip.h
// (whvi_fused_shs_bwd_f32; whvi_fused_shs_bwd_f16 / _bf16 for 16-bit activation streams).
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
//
// 16-bit activations (T = __half / __hip_bfloat16): x, grad_y and grad_x are 16-bit, everything else stays float32 -- the
// contract of fused16.hpp.  Elem<T>::unpack on the way in, the float32 chain above on the exactly-upcast values, ONE
// Elem<T>::pack when grad_x is stored, nothing rounded to 16 bits in between: grad_x is whvi_fused_shs_ex_f16 / _bf16
// (grad_y, a := c, b, c := a) and the sums are the float32 kernel's on the upcast operands.  A chunk holds 8 elements, so a
// tile of the same rows is half the chunks per lane (K = 2, 2, 2, 2, 2, 4, 8 for D = 64 .. 4096), the grid, the slots and the
// finishing launch are the float32 kernel's, and from D = 512 up (a row fills at least one chunk per lane) every column is
// summed over the same rows in the same order: the same bits.  Below, a row is shorter than 64 chunks one size earlier
// (D < 512, 24 sums per lane), so the lanes of a column hold other rows than in the float32 kernel.  The staged vectors lie
// in fused16.hpp's split layout (the first halves of all chunks, then the second halves: both 16-byte reads of a chunk's
// eight factors are lane-contiguous), and the whole tile is packed before its first store.
#include "dispatch.hpp"

namespace whvi {

constexpr int FUSED_BWD_MIN_LOG2D = 6, FUSED_BWD_MAX_LOG2D = 12;
inline bool fused_bwd_supported(int log2d) { return log2d >= FUSED_BWD_MIN_LOG2D && log2d <= FUSED_BWD_MAX_LOG2D; }

// chunks per lane of one wave tile: one row from D = 1024 up (4, 8, 16), 1024 floats (2 .. 16 rows) below; vec = elements of
// a 16-byte chunk (8 for 16-bit activations: the same rows in half the chunks)
constexpr int fused_bwd_k(int log2d, int vec = 4) { return (log2d >= 10 ? 1 << (log2d - 8) : 4) * 4 / vec; }
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

// the two transforms of the pipeline as fused_shs_kernel (VEC = 4) / fused_shs16_kernel (VEC = 8) issue them: FIRST from sign
// mask 0 (leaves SIGN_MID), the second from SIGN_MID (leaves 0)
template <int LOG2D, int K, bool FIRST, int VEC>
__device__ __forceinline__ void fused_bwd_fwht(float (&r)[K][VEC], int lane)
{
    constexpr int SIGN_MID = fwht_sign_out<VEC, LOG2D>(0);
    static_assert(fwht_sign_out<VEC, LOG2D>(SIGN_MID) == 0, "two transforms restore the sign convention");
    fwht_tile<float, VEC, K, LOG2D, POLICY_DPP, FUSED_PKMASK, true, FIRST ? 0 : SIGN_MID>(r, lane);
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

// the VEC float32 factors of one chunk as they come out of LDS: one 16-byte read (VEC = 4), or two (VEC = 8, split layout)
template <int VEC>
struct FusedBwdFactors {
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 q[VEC / 4];
    __device__ __forceinline__ float operator[](int e) const { return q[e >> 2][e & 3]; }
};

// part : (n_samples * n_slabs) slots of 3 D floats.  gx (n_samples * stride, D) or NULL; gy likewise; x the same, or
// (stride, D) with x_shared (WHVI_FUSED_SRC_SHARED: row r of every sample reads x[r]).  a, c : (D); b : (n_samples, D).
// NT: gy is read and gx written with the non-temporal policy (streams larger than the Infinity Cache).
// T: the storage type of x, gy and gx (float, __half, __hip_bfloat16); a, b, c, part are float32 throughout.
template <typename T, int LOG2D, int K, bool NT>
__global__ void __launch_bounds__(256)
fused_shs_bwd_kernel(float *__restrict__ part, u32x4 *__restrict__ gx, const u32x4 *__restrict__ gy, const u32x4 *__restrict__ x,
                     const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ c, uint32_t stride,
                     uint32_t slab_rows, uint32_t n_slabs, uint32_t x_shared)
{
    using E = Elem<T>;
    constexpr int VEC = E::VEC;
    static_assert(std::is_same<typename E::acc, float>::value && (VEC == 4 || VEC == 8), "float32 arithmetic on 4- or 2-byte storage");
    constexpr int D = 1 << LOG2D, SH = LOG2D - ilog2(VEC);  // SH = log2(chunks per row)
    constexpr uint32_t CPR = 1u << SH;
    constexpr bool WIDE = SH >= 6;                          // a row fills at least one chunk per lane
    constexpr int NC = WIDE ? (int)CPR / 64 : 1;            // column chunks per lane
    constexpr uint32_t RPT = (uint32_t)(K * 64) >> SH;      // rows per tile
    constexpr bool KEEP_X = K * VEC <= 16;                  // the x tile stays in registers for grad_c (D >= 2048 reads it again: L2)
    static_assert(K * 64 >= (int)CPR && K % NC == 0, "a tile holds whole rows");
    static_assert(K == fused_bwd_k(LOG2D, VEC), "the tile of fused_bwd_geom");
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef FusedBwdFactors<VEC> factors_t;
    extern __shared__ __attribute__((aligned(16))) float fused_bwd_lds[];
    float *const la = fused_bwd_lds, *const lb = la + D, *const lc = lb + D;

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t r_begin = slab * slab_rows, r_end = r_begin + slab_rows < stride ? r_begin + slab_rows : stride;
    // piece i of a vector (16 bytes) goes to piece j: in place, or -- 8 factors per chunk -- half (i & 1) of chunk i >> 1 in the
    // split layout
    constexpr uint32_t QUADS = (uint32_t)D / 4;
    for (uint32_t i = threadIdx.x; i < QUADS; i += 256) {
        const uint32_t j = VEC == 4 ? i : (i & 1) * (QUADS / 2) + (i >> 1);
        reinterpret_cast<f4 *>(la)[j] = reinterpret_cast<const f4 *>(a)[i];
        reinterpret_cast<f4 *>(lb)[j] = reinterpret_cast<const f4 *>(b + ((size_t)s << LOG2D))[i];
        reinterpret_cast<f4 *>(lc)[j] = reinterpret_cast<const f4 *>(c)[i];
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
    // the factors of the lane's chunk k of a staged vector
    auto factors = [&](const float *v, int k) __attribute__((always_inline)) -> factors_t {
        factors_t f;
        f.q[0] = reinterpret_cast<const f4 *>(v)[colq(k)];
        if constexpr (VEC == 8) f.q[1] = reinterpret_cast<const f4 *>(v + D / 2)[colq(k)];
        return f;
    };
    const size_t sample_row0 = (size_t)s * stride;
    const size_t x_row0 = x_shared ? 0 : sample_row0;

    float acc_a[NC][VEC], acc_b[NC][VEC], acc_c[NC][VEC];
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc_a[j][e] = acc_b[j][e] = acc_c[j][e] = 0.0f;

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
        float r[K][VEC], t1[K][VEC], xk[KEEP_X ? K : 1][VEC];
        u32x4 pre[K];
        // ---- t1 = H(c x)
#pragma unroll
        for (int k = 0; k < K; ++k) pre[k] = ld16<false>(xt + rel(k));
        phase_fence();
#pragma unroll
        for (int k = 0; k < K; ++k) {
            E::unpack(pre[k], r[k]);
            const factors_t cv = factors(lc, k);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
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
            const factors_t bv = factors(lb, k);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                t1[k][e] = r[k][e];
                r[k][e] = bv[e] * r[k][e];
            }
        }
        fused_bwd_fwht<LOG2D, K, false>(r, lane);
        phase_fence();
        // ---- grad_a += grad_y u;  v = H(a grad_y)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float gv[VEC];
            E::unpack(pre[k], gv);
            const factors_t av = factors(la, k);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
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
            const factors_t bv = factors(lb, k);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
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
                if (row_ok(k)) fused_bwd_acc(acc_c[k % NC][e], r[k][e], xv[e]);
                r[k][e] = cv[e] * r[k][e];
            }
            if constexpr (VEC == 4)
                if (gx != nullptr && row_ok(k)) st16<NT>(gxt + rel(k), E::pack(r[k]));
        }
        if constexpr (VEC == 8) {
            // 16-bit storage: the whole tile is rounded and packed first, into registers of its own, and only then stored -- no
            // pack writes a register that a store issued just before it still reads (fused16.hpp)
            u32x4 packed[K];
#pragma unroll
            for (int k = 0; k < K; ++k) packed[k] = E::pack(r[k]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (gx != nullptr && row_ok(k)) st16<NT>(gxt + rel(k), packed[k]);
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
        for (int e = 0; e < VEC; ++e)
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
                for (int e = 0; e < VEC; ++e) {
                    const uint32_t n = VEC * q + e;
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

// ---- host side: one checked call = the launch above plus the finishing launch.  The checks and the finishing launch are
// compiled once (fused_bwd_f32.hip); every storage type's translation unit instantiates its own kernels through
// fused_bwd_run<T>.
struct FusedBwdArgs {
    void *grad_x, *work;
    const void *grad_y, *x, *a, *b, *c;
    int64_t n_samples, sample_stride;
    int32_t log2d;
    bool x_shared, nt;
    FusedBwdGeom geom;
};

// Every argument check of whvi_fused_shs_bwd_*, before any device call; act_bytes = bytes of one element of x, grad_y and
// grad_x.  WHVI_OK with launch = false: nothing to launch.
int fused_bwd_check(FusedBwdArgs &r, bool &launch, void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *work,
                    const void *grad_y, const void *x, const void *a, const void *b, const void *c, int64_t S, int64_t stride,
                    int32_t log2d, int32_t flags, int64_t act_bytes);
// fused_shs_bwd_finish_kernel on the slots of r's grid
int fused_bwd_finish(const FusedBwdArgs &r, void *grad_a, void *grad_b, void *grad_c, hipStream_t st);

template <typename T, int L>
inline void fused_bwd_launch_one(const FusedBwdArgs &a, hipStream_t st)
{
    constexpr int K = fused_bwd_k(L, Elem<T>::VEC);
    const dim3 grid((unsigned)(a.n_samples * a.geom.n_slabs));
    const size_t lds = (size_t)fused_bwd_part_floats(L) * sizeof(float);
    note_launch<T>("fused_shs_bwd_kernel", L, K, a.nt);
#define WHVI_FUSED_BWD(NT)                                                                                              \
    hipLaunchKernelGGL((fused_shs_bwd_kernel<T, L, K, NT>), grid, dim3(256), lds, st, (float *)a.work, (u32x4 *)a.grad_x, \
                       (const u32x4 *)a.grad_y, (const u32x4 *)a.x, (const float *)a.a, (const float *)a.b, (const float *)a.c, \
                       (uint32_t)a.sample_stride, (uint32_t)a.geom.slab_rows, (uint32_t)a.geom.n_slabs, a.x_shared ? 1u : 0u)
    if (a.nt) WHVI_FUSED_BWD(true);
    else WHVI_FUSED_BWD(false);
#undef WHVI_FUSED_BWD
}

template <typename T>
inline int fused_bwd_run(void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *work, const void *grad_y, const void *x,
                         const void *a, const void *b, const void *c, int64_t n_samples, int64_t sample_stride, int32_t log2d,
                         int32_t flags, void *stream)
{
    FusedBwdArgs r;
    bool launch = false;
    int rc = fused_bwd_check(r, launch, grad_x, grad_a, grad_b, grad_c, work, grad_y, x, a, b, c, n_samples, sample_stride, log2d,
                             flags, (int64_t)sizeof(T));
    if (rc != WHVI_OK || !launch) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (log2d) {
    case 6: fused_bwd_launch_one<T, 6>(r, st); break;
    case 7: fused_bwd_launch_one<T, 7>(r, st); break;
    case 8: fused_bwd_launch_one<T, 8>(r, st); break;
    case 9: fused_bwd_launch_one<T, 9>(r, st); break;
    case 10: fused_bwd_launch_one<T, 10>(r, st); break;
    case 11: fused_bwd_launch_one<T, 11>(r, st); break;
    default: fused_bwd_launch_one<T, 12>(r, st); break;
    }
    rc = after_launch("fused_shs_bwd");
    if (rc != WHVI_OK) return rc;
    return fused_bwd_finish(r, grad_a, grad_b, grad_c, st);
}

}  // namespace whvi
