#pragma once
// whvi_amd/csrc/fused_stacked_layer.hpp -- the rectangular fastfood LAYER in one launch: fused_shs_stacked_kernel's J square
// operators on the same rows (fused_stacked.hpp), with what a network puts around them folded into the same pass -- the
// activation in front, the bias, the activation behind, and the narrowing to n_cols <= J D columns at a row pitch of the
// caller's.  ABI: include/whvi_hip.h (whvi_fused_shs_stacked_layer_f32).
//
//     dst[r ld_dst + j D + n] = act_out(a[j, n] * H(b[j, s(r), :] (.) H(c[j, :] (.) act_in(src[r, :])))[n] + bias[j D + n])
//
// for j D + n < n_cols; nothing else of dst is written.  act_in / act_out: relu_ (diag_apply.hpp: NaN passes, as in torch.relu)
// or the identity, chosen by the option word -- a runtime, wave-uniform argument, as in diag_apply_kernel.  The bias add is a
// rounding of its own behind the a multiply and is skipped (not "+ 0") without a bias.
//
// Arithmetic, geometry, tile layout, the rolled j loop, the packed tile behind a scheduling barrier, the compiler-emitted
// 16-byte stores and the clamped duplicate rows of partial tiles are fused_shs_stacked_kernel's: with no option, no bias and
// n_cols == ld_dst == J D the result has its bits.  The bias is staged in LDS behind the J triples: (12 + 4 [bias]) D J bytes.
// A 16-byte chunk whose first column is >= n_cols is computed (every lane takes part in the transforms) and not stored;
// n_cols % 4 == 0, so no chunk straddles the edge.  No atomics, no scratch, no allocation, no synchronisation.
#include "diag_apply.hpp"
#include "dispatch.hpp"
#include "fused_bwd.hpp"
#include "fused_stacked.hpp"

namespace whvi {

constexpr uint32_t STACKED_OPT_RELU_IN = 1u, STACKED_OPT_RELU_OUT = 2u, STACKED_OPT_BIAS = 4u;

inline bool fused_stacked_layer_supported(int log2d, int64_t n_blocks, bool has_bias)
{
    if (log2d < FUSED_STACKED_MIN_LOG2D || log2d > FUSED_STACKED_MAX_LOG2D || n_blocks < 1) return false;
    return n_blocks <= FUSED_STACKED_LDS_BYTES / ((int64_t)(has_bias ? 16 : 12) << log2d);
}

// dst : n_samples * stride rows of pitch ld_q chunks, columns 0 .. 4 n_colq - 1 written.  src, a, b, c : as in
// fused_shs_stacked_kernel.  bias : (J D), read only with STACKED_OPT_BIAS.  LDS: J triples [a_j | b_{j,s} | c_j], then the bias.
template <typename T, int LOG2D, int K, bool NT>
__global__ void __launch_bounds__(256)
fused_shs_stacked_layer_kernel(u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, const float *__restrict__ a,
                               const float *__restrict__ b, const float *__restrict__ c, const float *__restrict__ bias, uint32_t J,
                               uint32_t n_samples, uint32_t stride, uint32_t slab_rows, uint32_t n_slabs, uint32_t src_shared,
                               uint32_t n_colq, uint32_t ld_q, uint32_t opts)
{
    using E = Elem<T>;
    constexpr int VEC = E::VEC;
    static_assert(std::is_same<T, float>::value && VEC == 4, "float32 storage");
    constexpr int D = 1 << LOG2D, SH = LOG2D - 2;          // SH = log2(chunks per row)
    constexpr uint32_t CPR = 1u << SH;
    constexpr bool WIDE = SH >= 6;                          // a row fills at least one chunk per lane
    constexpr int NC = WIDE ? (int)CPR / 64 : 1;            // column chunks per lane
    constexpr uint32_t RPT = (uint32_t)(K * 64) >> SH;      // rows per tile
    static_assert(K * 64 >= (int)CPR && K % NC == 0, "a tile holds whole rows");
    static_assert(K == fused_bwd_k(LOG2D, VEC), "the tile of fused_bwd_geom");
    typedef float f4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float fused_stacked_layer_lds[];
    const bool relu_in = (opts & STACKED_OPT_RELU_IN) != 0, relu_out = (opts & STACKED_OPT_RELU_OUT) != 0;
    const bool has_bias = (opts & STACKED_OPT_BIAS) != 0;   // (all three wave-uniform: kernel arguments)

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t r_begin = slab * slab_rows;
    const uint32_t r_end = (uint64_t)r_begin + slab_rows < stride ? r_begin + slab_rows : stride;
    constexpr uint32_t QUADS = (uint32_t)D / 4;
    for (uint32_t j = 0; j < J; ++j) {
        f4 *const la = reinterpret_cast<f4 *>(fused_stacked_layer_lds + (size_t)3 * j * D);
        const f4 *const ga = reinterpret_cast<const f4 *>(a + ((size_t)j << LOG2D));
        const f4 *const gb = reinterpret_cast<const f4 *>(b + (((size_t)j * n_samples + s) << LOG2D));
        const f4 *const gc = reinterpret_cast<const f4 *>(c + ((size_t)j << LOG2D));
        for (uint32_t i = threadIdx.x; i < QUADS; i += 256) {
            la[i] = ga[i];
            la[QUADS + i] = gb[i];
            la[2 * QUADS + i] = gc[i];
        }
    }
    f4 *const lbias = reinterpret_cast<f4 *>(fused_stacked_layer_lds + (size_t)3 * J * D);      // (J D) floats, with a bias only
    if (has_bias) {
        const f4 *const gbias = reinterpret_cast<const f4 *>(bias);
        for (uint32_t i = threadIdx.x; i < J * QUADS; i += 256) lbias[i] = gbias[i];
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
    const size_t src_row0 = src_shared ? 0 : sample_row0;

    // One tile: rows rt .. rt + RPT - 1.  TAIL (tiles of several rows only): rows past the slab's end are clamped duplicates --
    // computed (every lane takes part in the transforms), never stored.
    auto tile = [&](uint32_t rt, auto tail) __attribute__((always_inline)) {
        constexpr bool TAIL = decltype(tail)::value != 0;
        auto row_ok = [&](int k) __attribute__((always_inline)) -> bool { return !TAIL || rt + row_in(k) < r_end; };
        auto rel = [&](int k) __attribute__((always_inline)) -> uint32_t {
            if constexpr (!TAIL) return (uint32_t)(k * 64 + lane);
            else return ((row_ok(k) ? row_in(k) : r_end - 1 - rt) << SH) + colq(k);
        };
        const u32x4 *const xt = src + ((src_row0 + rt) << SH);
        u32x4 pre[K];
        if (src_shared) {                                    // (wave-uniform) a shared source is cache-resident by intent
#pragma unroll
            for (int k = 0; k < K; ++k) pre[k] = ld16<false>(xt + rel(k));
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) pre[k] = ld16<NT>(xt + rel(k));
        }
        if (relu_in) {                                       // the activation in FRONT of the layer: once per tile, before the per-j copy
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float v[VEC];
                E::unpack(pre[k], v);
#pragma unroll
                for (int e = 0; e < VEC; ++e) v[e] = relu_(v[e]);
                pre[k] = E::pack(v);
            }
        }
        // chunk k of segment 0 of the lane's output rows, in chunks from dst
        size_t out[K];
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = (sample_row0 + rt + row_in(k)) * ld_q + colq(k);
#pragma unroll 1
        for (uint32_t j = 0; j < J; ++j) {
            const f4 *const la = reinterpret_cast<const f4 *>(fused_stacked_layer_lds + (size_t)3 * j * D);
            const f4 *const lb = la + QUADS, *const lc = lb + QUADS;
            float r[K][VEC];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                E::unpack(pre[k], r[k]);
                const f4 cv = lc[colq(k)];
#pragma unroll
                for (int e = 0; e < VEC; ++e) r[k][e] = cv[e] * r[k][e];
            }
            fused_bwd_fwht<LOG2D, K, true>(r, lane);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const f4 bv = lb[colq(k)];
#pragma unroll
                for (int e = 0; e < VEC; ++e) r[k][e] = bv[e] * r[k][e];
            }
            fused_bwd_fwht<LOG2D, K, false>(r, lane);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const f4 av = la[colq(k)];
#pragma unroll
                for (int e = 0; e < VEC; ++e) r[k][e] = av[e] * r[k][e];
            }
            if (has_bias) {                                  // a rounding of its own behind the a multiply
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const f4 hv = lbias[j * QUADS + colq(k)];
#pragma unroll
                    for (int e = 0; e < VEC; ++e) r[k][e] = r[k][e] + hv[e];
                }
            }
            if (relu_out) {                                  // the activation BEHIND the layer, applied before the store
#pragma unroll
                for (int k = 0; k < K; ++k)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) r[k][e] = relu_(r[k][e]);
            }
            // the whole tile is packed first, into registers of its own, and only then stored
            u32x4 packed[K];
#pragma unroll
            for (int k = 0; k < K; ++k) packed[k] = E::pack(r[k]);
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t colq0 = j << SH;                  // segment j's first chunk of the row
            if (colq0 + CPR <= n_colq) {                     // (wave-uniform) a whole segment: fused_shs_stacked_kernel's run of stores
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (row_ok(k)) st16<NT>(dst + out[k] + colq0, packed[k]);
            } else {                                         // the narrowed last segment: chunks from n_cols on are not stored
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (row_ok(k) && colq0 + colq(k) < n_colq) st16<NT>(dst + out[k] + colq0, packed[k]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // the loop bound is wave-uniform: every lane of the wave takes part in the DPP / permlane stages of the transforms
    for (uint32_t rt = r_begin + (uint32_t)wave * RPT; rt < r_end; rt += 4 * RPT) {
        if constexpr (RPT > 1) {
            if (rt + RPT <= r_end) tile(rt, IC<0>{});
            else tile(rt, IC<1>{});
        } else {
            tile(rt, IC<0>{});
        }
    }
}

// ---- host side
struct FusedStackedLayerArgs {
    void *dst;
    const void *src, *a, *b, *c, *bias;
    int64_t n_blocks, n_samples, sample_stride, n_cols, ld_dst;
    int32_t log2d;
    uint32_t opts;
    bool src_shared, nt;
    FusedBwdGeom geom;
};

template <typename T, int L>
inline void fused_stacked_layer_launch_one(const FusedStackedLayerArgs &r, hipStream_t st)
{
    constexpr int K = fused_bwd_k(L, Elem<T>::VEC);
    const dim3 grid((unsigned)(r.n_samples * r.geom.n_slabs));
    const size_t lds = (size_t)r.n_blocks * (r.bias ? 4 : 3) * sizeof(float) << L;
    note_launch<T>("fused_shs_stacked_layer_kernel", L, K, r.nt);
#define WHVI_FUSED_STACKED_LAYER(NT)                                                                                    \
    hipLaunchKernelGGL((fused_shs_stacked_layer_kernel<T, L, K, NT>), grid, dim3(256), lds, st, (u32x4 *)r.dst,         \
                       (const u32x4 *)r.src, (const float *)r.a, (const float *)r.b, (const float *)r.c, (const float *)r.bias, \
                       (uint32_t)r.n_blocks, (uint32_t)r.n_samples, (uint32_t)r.sample_stride, (uint32_t)r.geom.slab_rows, \
                       (uint32_t)r.geom.n_slabs, r.src_shared ? 1u : 0u, (uint32_t)(r.n_cols / 4), (uint32_t)(r.ld_dst / 4), r.opts)
    if (r.nt) WHVI_FUSED_STACKED_LAYER(true);
    else WHVI_FUSED_STACKED_LAYER(false);
#undef WHVI_FUSED_STACKED_LAYER
}

}  // namespace whvi
