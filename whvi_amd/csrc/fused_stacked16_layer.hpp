#pragma once
// whvi_amd/csrc/fused_stacked16_layer.hpp -- the rectangular fastfood LAYER in one launch for 16-bit ACTIVATION storage (__half /
// __hip_bfloat16) with float32 scale vectors and a float32 bias: fused_stacked16_kernel (fused_stacked16.hpp) with the epilogue
// of fused_shs_stacked_layer_kernel (fused_stacked_layer.hpp) -- the activation in front, the bias, the activation behind, and
// the narrowing to n_cols <= J D columns at a row pitch of the caller's.  ABI: include/whvi_hip.h
// (whvi_fused_shs_stacked_layer_f16 / _bf16).
//
//     dst[r ld_dst + j D + n] = pack(act_out(a[j, n] * H(b[j, s(r), :] (.) H(c[j, :] (.) act_in(unpack(src[r, :]))))[n] + bias[j D + n]))
//
// for j D + n < n_cols; nothing else of dst is written.  act_in / act_out: relu_ (diag_apply.hpp: NaN passes, as in torch.relu)
// or the identity, chosen by the option word -- a runtime, wave-uniform argument.  A sibling of both kernels, not another
// instantiation of either: their symbols are pinned.
//
// Contract (fused16.hpp's): Elem<T>::unpack in, every multiply its own float32 rounding, float32 butterflies in the forward's
// sign sequence, the float32 bias added in float32 as a rounding of its own behind the a multiply (skipped, not "+ 0", without
// a bias), ONE Elem<T>::pack when an element is stored, nothing rounded to 16 bits in between.  act_in is applied to the
// unpacked values for every j (the packed tile is what stays in registers; the values are those of one application per tile).
// With no option, no bias and n_cols == ld_dst == J D the result has fused_stacked16_kernel's bits.
//
// Geometry: fused_stacked16_kernel's.  A block of four waves owns (sample s, a slab of that sample's rows) -- fused_bwd_geom --
// stages all J triples a_j, b_{j,s}, c_j in LDS once in fused16.hpp's split layout and, behind them, the bias, block by block
// in the same split layout (its eight addends per chunk are two lane-contiguous 16-byte reads): (12 + 4 [bias]) D J bytes.
// The j loop is rolled, the whole tile is packed behind a scheduling barrier and only then stored.  A 16-byte chunk (8
// columns) whose first column is >= n_cols is computed (every lane takes part in the transforms) and not stored; n_cols % 8
// == 0, so no chunk straddles the edge; a segment wholly inside n_cols (a wave-uniform test) keeps the unpredicated run of
// stores.  No atomics, no scratch, no allocation, no synchronisation.
#include "diag_apply.hpp"
#include "dispatch.hpp"
#include "fused_bwd.hpp"
#include "fused_stacked.hpp"
#include "fused_stacked_layer.hpp"

namespace whvi {

// the float32 layer's rule: the staged vectors and the bias are float32 whatever the activations are stored in
inline bool fused_stacked16_layer_supported(int log2d, int64_t n_blocks, bool has_bias)
{
    return fused_stacked_layer_supported(log2d, n_blocks, has_bias);
}

// dst : n_samples * stride rows of T at a pitch of ld_q chunks, columns 0 .. 8 n_colq - 1 written.  src, a, b, c : as in
// fused_stacked16_kernel.  bias : (J D) float32, read only with STACKED_OPT_BIAS.  LDS: J triples [a_j | b_{j,s} | c_j], then the
// J blocks of the bias, each vector in the split layout.
// NT: the streamed accesses (the stores, and the loads of a source of its own) take the non-temporal policy.
template <typename T, int LOG2D, int K, bool NT>
__global__ void __launch_bounds__(256)
fused_stacked16_layer_kernel(u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, const float *__restrict__ a,
                             const float *__restrict__ b, const float *__restrict__ c, const float *__restrict__ bias, uint32_t J,
                             uint32_t n_samples, uint32_t stride, uint32_t slab_rows, uint32_t n_slabs, uint32_t src_shared,
                             uint32_t n_colq, uint32_t ld_q, uint32_t opts)
{
    using E = Elem<T>;
    constexpr int VEC = E::VEC;
    static_assert(sizeof(T) == 2 && VEC == 8 && std::is_same<typename E::acc, float>::value, "16-bit storage, float32 arithmetic");
    constexpr int D = 1 << LOG2D, SH = LOG2D - 3;          // SH = log2(chunks per row)
    constexpr uint32_t CPR = 1u << SH;
    constexpr bool WIDE = SH >= 6;                          // a row fills at least one chunk per lane
    constexpr int NC = WIDE ? (int)CPR / 64 : 1;            // column chunks per lane
    constexpr uint32_t RPT = (uint32_t)(K * 64) >> SH;      // rows per tile
    static_assert(K * 64 >= (int)CPR && K % NC == 0, "a tile holds whole rows");
    static_assert(K == fused_bwd_k(LOG2D, VEC), "the tile of fused_bwd_geom");
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef FusedBwdFactors<VEC> factors_t;
    extern __shared__ __attribute__((aligned(16))) float fused_stacked16_layer_lds[];
    const bool relu_in = (opts & STACKED_OPT_RELU_IN) != 0, relu_out = (opts & STACKED_OPT_RELU_OUT) != 0;
    const bool has_bias = (opts & STACKED_OPT_BIAS) != 0;   // (all three wave-uniform: kernel arguments)

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t r_begin = slab * slab_rows;
    const uint32_t r_end = (uint64_t)r_begin + slab_rows < stride ? r_begin + slab_rows : stride;
    // piece i of a vector (16 bytes) is half (i & 1) of chunk i >> 1: it goes to piece (i & 1) * QUADS / 2 + (i >> 1)
    constexpr uint32_t QUADS = (uint32_t)D / 4;
    for (uint32_t j = 0; j < J; ++j) {
        f4 *const la = reinterpret_cast<f4 *>(fused_stacked16_layer_lds + (size_t)3 * j * D);
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
    float *const lbias = fused_stacked16_layer_lds + (size_t)3 * J * D;      // J blocks of D floats, with a bias only
    if (has_bias) {
        const f4 *const gbias = reinterpret_cast<const f4 *>(bias);
        for (uint32_t i = threadIdx.x; i < J * QUADS; i += 256) {
            const uint32_t ii = i & (QUADS - 1);                             // piece ii of block i / QUADS
            reinterpret_cast<f4 *>(lbias)[(i - ii) + (ii & 1) * (QUADS / 2) + (ii >> 1)] = gbias[i];
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
    // the eight factors of the lane's chunk k of a staged vector
    auto factors = [&](const float *v, int k) __attribute__((always_inline)) -> factors_t {
        factors_t f;
        f.q[0] = reinterpret_cast<const f4 *>(v)[colq(k)];
        f.q[1] = reinterpret_cast<const f4 *>(v + D / 2)[colq(k)];
        return f;
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
        // chunk k of segment 0 of the lane's output rows, in chunks from dst
        size_t out[K];
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = (sample_row0 + rt + row_in(k)) * ld_q + colq(k);
#pragma unroll 1
        for (uint32_t j = 0; j < J; ++j) {
            const float *const la = fused_stacked16_layer_lds + (size_t)3 * j * D;
            const float *const lb = la + D, *const lc = lb + D;
            float r[K][VEC];
#pragma unroll
            for (int k = 0; k < K; ++k) E::unpack(pre[k], r[k]);
            if (relu_in) {                                   // the activation in FRONT of the layer, on the unpacked values
#pragma unroll
                for (int k = 0; k < K; ++k)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) r[k][e] = relu_(r[k][e]);
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const factors_t cv = factors(lc, k);
#pragma unroll
                for (int e = 0; e < VEC; ++e) r[k][e] = cv[e] * r[k][e];
            }
            fused_bwd_fwht<LOG2D, K, true>(r, lane);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const factors_t bv = factors(lb, k);
#pragma unroll
                for (int e = 0; e < VEC; ++e) r[k][e] = bv[e] * r[k][e];
            }
            fused_bwd_fwht<LOG2D, K, false>(r, lane);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const factors_t av = factors(la, k);
#pragma unroll
                for (int e = 0; e < VEC; ++e) r[k][e] = av[e] * r[k][e];
            }
            if (has_bias) {                                  // a float32 rounding of its own behind the a multiply
                const float *const lh = lbias + (size_t)j * D;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const factors_t hv = factors(lh, k);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) r[k][e] = r[k][e] + hv[e];
                }
            }
            if (relu_out) {                                  // the activation BEHIND the layer, applied before the one rounding
#pragma unroll
                for (int k = 0; k < K; ++k)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) r[k][e] = relu_(r[k][e]);
            }
            // the whole tile is rounded and packed first, into registers of its own, and only then stored -- no pack writes a
            // register that a store issued just before it still reads (fused16.hpp)
            u32x4 packed[K];
#pragma unroll
            for (int k = 0; k < K; ++k) packed[k] = E::pack(r[k]);
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t colq0 = j << SH;                  // segment j's first chunk of the row
            if (colq0 + CPR <= n_colq) {                     // (wave-uniform) a whole segment: fused_stacked16_kernel's run of stores
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

// ---- host side: the checks are compiled once (abi.hip); each storage type's translation unit instantiates its own kernels
// through fused_stacked16_layer_run<T>.

// Every argument check of whvi_fused_shs_stacked_layer_f16 / _bf16, before any device call (whvi_fused_shs_stacked_layer_f32's,
// in its order, with 2-byte activations and 8-column chunks).  WHVI_OK with launch = false: nothing to launch.
int fused_stacked16_layer_check(FusedStackedLayerArgs &r, bool &launch, void *dst, const void *src, const void *a, const void *b,
                                const void *c, const void *bias, int64_t J, int64_t S, int64_t stride, int32_t log2d,
                                int64_t n_cols, int64_t ld_dst, int32_t flags);

template <typename T, int L>
inline void fused_stacked16_layer_launch_one(const FusedStackedLayerArgs &r, hipStream_t st)
{
    constexpr int K = fused_bwd_k(L, Elem<T>::VEC);
    const dim3 grid((unsigned)(r.n_samples * r.geom.n_slabs));
    const size_t lds = (size_t)r.n_blocks * (r.bias ? 4 : 3) * sizeof(float) << L;
    note_launch<T>("fused_stacked16_layer_kernel", L, K, r.nt);
#define WHVI_FUSED_STACKED16_LAYER(NT)                                                                                  \
    hipLaunchKernelGGL((fused_stacked16_layer_kernel<T, L, K, NT>), grid, dim3(256), lds, st, (u32x4 *)r.dst,           \
                       (const u32x4 *)r.src, (const float *)r.a, (const float *)r.b, (const float *)r.c, (const float *)r.bias, \
                       (uint32_t)r.n_blocks, (uint32_t)r.n_samples, (uint32_t)r.sample_stride, (uint32_t)r.geom.slab_rows, \
                       (uint32_t)r.geom.n_slabs, r.src_shared ? 1u : 0u, (uint32_t)(r.n_cols / 8), (uint32_t)(r.ld_dst / 8), r.opts)
    if (r.nt) WHVI_FUSED_STACKED16_LAYER(true);
    else WHVI_FUSED_STACKED16_LAYER(false);
#undef WHVI_FUSED_STACKED16_LAYER
}

template <typename T>
inline int fused_stacked16_layer_run(void *dst, const void *src, const void *a, const void *b, const void *c, const void *bias,
                                     int64_t n_blocks, int64_t n_samples, int64_t sample_stride, int32_t log2d, int64_t n_cols,
                                     int64_t ld_dst, int32_t flags, void *stream)
{
    FusedStackedLayerArgs r;
    bool launch = false;
    const int rc = fused_stacked16_layer_check(r, launch, dst, src, a, b, c, bias, n_blocks, n_samples, sample_stride, log2d,
                                               n_cols, ld_dst, flags);
    if (rc != WHVI_OK || !launch) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (log2d) {
    case 6: fused_stacked16_layer_launch_one<T, 6>(r, st); break;
    case 7: fused_stacked16_layer_launch_one<T, 7>(r, st); break;
    case 8: fused_stacked16_layer_launch_one<T, 8>(r, st); break;
    case 9: fused_stacked16_layer_launch_one<T, 9>(r, st); break;
    case 10: fused_stacked16_layer_launch_one<T, 10>(r, st); break;
    default: fused_stacked16_layer_launch_one<T, 11>(r, st); break;
    }
    return after_launch("fused_shs_stacked_layer (16-bit)");
}

}  // namespace whvi
