#pragma once
// whvi_amd/csrc/fused_stacked_fwd.hpp -- the rectangular fastfood layer's forward pass: J independent square operators applied
// to the SAME rows, their outputs written side by side, in ONE launch -- for float32, __half and __hip_bfloat16 activation
// storage, with or without the layer's epilogue.  ONE body, fused_stacked_fwd<T, LOG2D, K, NT, LAYER>, behind four kernel
// names.  ABI: include/whvi_hip.h (whvi_fused_shs_stacked_f32 / _f16 / _bf16, whvi_fused_shs_stacked_layer_f32 / _f16 / _bf16).
//
//     dst[r, j D + n] = pack(a[j, n] * H(b[j, s(r), :] (.) H(c[j, :] (.) unpack(src[r, :])))[n]),       j = 0 .. J - 1
//
// i.e. block j of the (rows, J D) output is whvi_fused_shs_f32 / whvi_fused_shs_ex_f16 / _bf16(src, a[j], b[j], c[j], axis = COL)
// -- with a shared source, that launch on the expanded source; the paper's stacking of square S1 H diag(g) H S2 blocks
// (src/weights.py: WHVIStackedMatrix.setup_dimensions) -- without J launches that each read the row again and a concatenation
// that reads and writes all of it once more: a row is read once and J segments are written, (1 + J) D elements per row instead
// of about 4 J D.  LAYER folds what a network puts around the blocks into the same pass -- the activation in front, the bias,
// the activation behind, and the narrowing to n_cols <= J D columns at a row pitch of the caller's:
//
//     dst[r ld_dst + j D + n] = pack(act_out(a[j, n] * H(b[j, s(r), :] (.) H(c[j, :] (.) act_in(unpack(src[r, :]))))[n] + bias[j D + n]))
//
// for j D + n < n_cols; nothing else of dst is written.  act_in / act_out: relu_ (diag_apply.hpp: NaN passes, as in torch.relu)
// or the identity, chosen by the option word -- a runtime, wave-uniform argument, as in diag_apply_kernel.  The bias add is a
// rounding of its own behind the a multiply and is skipped (not "+ 0") without a bias.  With no option, no bias and n_cols ==
// ld_dst == J D the LAYER result has the bits of the plain one.
//
// What the body is parameterised on:
//   * T -> Elem<T>::VEC, the elements of a 16-byte chunk: 4 (float32) or 8 (16-bit storage: the same rows in half the chunks).
//     The staged float32 vectors lie in place for VEC = 4 and in fused16.hpp's split layout for VEC = 8 (the first halves of all
//     chunks, then the second halves: both 16-byte reads of a chunk's eight factors are lane-contiguous); FusedBwdFactors<VEC>
//     (fused_bwd.hpp) holds one read or two.  This is fused_shs_bwd_kernel's scheme.
//   * LAYER -> the epilogue and the narrowed store, and the output pitch (ld_q, or J D in chunks).
//   * where act_in is applied, the one place the storage types differ on purpose: float32 applies it ONCE per tile, on the packed
//     tile that stays in registers (pack and unpack are bit casts); 16-bit storage applies it for EVERY j on the unpacked values
//     (the packed tile is what stays in registers, and rounding relu(x) to 16 bits again would be a no-op the compiler does not
//     see): the values are those of one application per tile.
//
// Arithmetic: every multiply is its own float32 rounding and the two transforms are fwht_tile with fused_shs_kernel's template
// arguments and sign sequence (0 -> SIGN_MID -> 0), exactly as fused_bwd.hpp issues them (fused_bwd_fwht): segment j has, element
// for element, the value of the per-block launch (the sign of an exact zero exempt, as for that entry).  The 16-bit contract is
// fused16.hpp's: Elem<T>::unpack in, float32 throughout, the float32 bias added in float32, ONE Elem<T>::pack when an element is
// stored, nothing rounded to 16 bits in between.
//
// Geometry: fused_shs_bwd_kernel's.  A block of four waves owns (sample s, a slab of that sample's rows) -- fused_bwd_geom, a
// function of the arguments alone -- stages all J triples a_j, b_{j,s}, c_j in LDS once and, LAYER with a bias, the bias behind
// them, block by block in the same layout ((12 + 4 [bias]) D J bytes), and walks its slab one wave tile at a time, in
// fused_shs_kernel's chunk layout (chunk k * 64 + lane): K = fused_bwd_k(LOG2D, VEC) chunks per lane, one row for D >= 1024,
// 1024 / D rows below.  Per tile the input is loaded once and kept packed in registers; for each j it is unpacked, run through
// scale -> transform -> scale -> transform -> scale, the whole output tile is packed, and only then stored: D-wide segments at
// column offset j D.  The j loop is rolled.  LAYER: a 16-byte chunk whose first column is >= n_cols is computed (every lane
// takes part in the transforms) and not stored; n_cols is a multiple of VEC, so no chunk straddles the edge; a segment wholly
// inside n_cols (a wave-uniform test) keeps the unpredicated run of stores.  No atomics, no scratch, no allocation, no
// synchronisation.
//
// The four __global__ templates below are what the library ships and what whvi_last_kernel names: their names, parameter lists
// and translation units are pinned (tests/test_fastfood_stacked*_host.py, tools/slab_table.py), their bodies are one call.
#include "diag_apply.hpp"
#include "dispatch.hpp"
#include "fused_bwd.hpp"

namespace whvi {

constexpr int FUSED_STACKED_MIN_LOG2D = 6, FUSED_STACKED_MAX_LOG2D = 11;
constexpr int64_t FUSED_STACKED_LDS_BYTES = 65536;        // whvi_mlp_apply_supported's budget
constexpr uint32_t STACKED_OPT_RELU_IN = 1u, STACKED_OPT_RELU_OUT = 2u, STACKED_OPT_BIAS = 4u;

// The staged vectors and the bias are float32 whatever the activations are stored in: one rule for every storage type.
inline bool fused_stacked_layer_supported(int log2d, int64_t n_blocks, bool has_bias)
{
    if (log2d < FUSED_STACKED_MIN_LOG2D || log2d > FUSED_STACKED_MAX_LOG2D || n_blocks < 1) return false;
    return n_blocks <= FUSED_STACKED_LDS_BYTES / ((int64_t)(has_bias ? 16 : 12) << log2d);
}
inline bool fused_stacked_supported(int log2d, int64_t n_blocks) { return fused_stacked_layer_supported(log2d, n_blocks, false); }

// dst : n_samples * stride rows of T; plain, (rows, J D); LAYER, at a pitch of ld_q chunks, columns 0 .. VEC n_colq - 1 written.
// src : the same rows of D, or (stride, D) with src_shared (row r of every sample reads src[r]).  a, c : (J, D) float32;
// b : (J, n_samples, D) float32.  bias : (J D) float32, read only with STACKED_OPT_BIAS.  bias, n_colq, ld_q, opts : LAYER only.
// lds : J triples [a_j | b_{j,s} | c_j] of D floats, then (LAYER, with a bias) the J blocks of the bias.
// NT: the streamed accesses (the stores, and the loads of a source of its own) take the non-temporal policy.
template <typename T, int LOG2D, int K, bool NT, bool LAYER>
__device__ __forceinline__ void
fused_stacked_fwd(float *lds, u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, const float *__restrict__ a,
                  const float *__restrict__ b, const float *__restrict__ c, const float *__restrict__ bias, uint32_t J,
                  uint32_t n_samples, uint32_t stride, uint32_t slab_rows, uint32_t n_slabs, uint32_t src_shared, uint32_t n_colq,
                  uint32_t ld_q, uint32_t opts)
{
    using E = Elem<T>;
    constexpr int VEC = E::VEC;
    static_assert(std::is_same<typename E::acc, float>::value && (VEC == 4 || VEC == 8), "float32 arithmetic on 4- or 2-byte storage");
    constexpr int D = 1 << LOG2D, SH = LOG2D - ilog2(VEC);  // SH = log2(chunks per row)
    constexpr uint32_t CPR = 1u << SH;
    constexpr bool WIDE = SH >= 6;                          // a row fills at least one chunk per lane
    constexpr int NC = WIDE ? (int)CPR / 64 : 1;            // column chunks per lane
    constexpr uint32_t RPT = (uint32_t)(K * 64) >> SH;      // rows per tile
    static_assert(K * 64 >= (int)CPR && K % NC == 0, "a tile holds whole rows");
    static_assert(K == fused_bwd_k(LOG2D, VEC), "the tile of fused_bwd_geom");
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef FusedBwdFactors<VEC> factors_t;
    // where act_in is applied (the header's third point): on the packed tile, once; or on the unpacked values, for every j
    constexpr bool RELU_IN_PER_TILE = LAYER && VEC == 4, RELU_IN_PER_J = LAYER && VEC == 8;
    // the epilogue's switches, looked at under if constexpr (LAYER) only (all three wave-uniform: kernel arguments)
    const bool relu_in = (opts & STACKED_OPT_RELU_IN) != 0, relu_out = (opts & STACKED_OPT_RELU_OUT) != 0;
    const bool has_bias = (opts & STACKED_OPT_BIAS) != 0;

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t r_begin = slab * slab_rows;
    const uint32_t r_end = (uint64_t)r_begin + slab_rows < stride ? r_begin + slab_rows : stride;
    // piece i of a vector (16 bytes) goes to piece q: in place, or -- 8 factors per chunk -- half (i & 1) of chunk i >> 1 in the
    // split layout.  (Written out in both loops: behind a lambda the compiler unrolls the j loop differently.)
    constexpr uint32_t QUADS = (uint32_t)D / 4;
    for (uint32_t j = 0; j < J; ++j) {
        f4 *const la = reinterpret_cast<f4 *>(lds + (size_t)3 * j * D);
        const f4 *const ga = reinterpret_cast<const f4 *>(a + ((size_t)j << LOG2D));
        const f4 *const gb = reinterpret_cast<const f4 *>(b + (((size_t)j * n_samples + s) << LOG2D));
        const f4 *const gc = reinterpret_cast<const f4 *>(c + ((size_t)j << LOG2D));
        for (uint32_t i = threadIdx.x; i < QUADS; i += 256) {
            const uint32_t q = VEC == 4 ? i : (i & 1) * (QUADS / 2) + (i >> 1);
            la[q] = ga[i];
            la[QUADS + q] = gb[i];
            la[2 * QUADS + q] = gc[i];
        }
    }
    float *const lbias = lds + (size_t)3 * J * D;           // J blocks of D floats, with a bias only
    if constexpr (LAYER) {
        if (has_bias) {
            const f4 *const gbias = reinterpret_cast<const f4 *>(bias);
            for (uint32_t i = threadIdx.x; i < J * QUADS; i += 256) {
                const uint32_t ii = i & (QUADS - 1);        // piece ii of block i / QUADS
                reinterpret_cast<f4 *>(lbias)[VEC == 4 ? i : (i - ii) + (ii & 1) * (QUADS / 2) + (ii >> 1)] = gbias[i];
            }
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
    // the factors of the lane's chunk k of a staged vector
    auto factors = [&](const float *v, int k) __attribute__((always_inline)) -> factors_t {
        factors_t f;
        f.q[0] = reinterpret_cast<const f4 *>(v)[colq(k)];
        if constexpr (VEC == 8) f.q[1] = reinterpret_cast<const f4 *>(v + D / 2)[colq(k)];
        return f;
    };
    const size_t sample_row0 = (size_t)s * stride;
    const size_t src_row0 = src_shared ? 0 : sample_row0;
    const size_t pitch = LAYER ? (size_t)ld_q : (size_t)J << SH;             // chunks of one output row

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
        if constexpr (RELU_IN_PER_TILE) {
            if (relu_in) {                                   // the activation in FRONT of the layer: once per tile, before the per-j copy
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    float v[VEC];
                    E::unpack(pre[k], v);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) v[e] = relu_(v[e]);
                    pre[k] = E::pack(v);
                }
            }
        }
        // chunk k of segment 0 of the lane's output rows, in chunks from dst
        size_t out[K];
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = (sample_row0 + rt + row_in(k)) * pitch + colq(k);
#pragma unroll 1
        for (uint32_t j = 0; j < J; ++j) {
            const float *const la = lds + (size_t)3 * j * D;
            const float *const lb = la + D, *const lc = lb + D;
            float r[K][VEC];
            if constexpr (RELU_IN_PER_J) {                   // (otherwise a chunk is unpacked where it is first scaled)
#pragma unroll
                for (int k = 0; k < K; ++k) E::unpack(pre[k], r[k]);
                if (relu_in) {                               // the activation in FRONT of the layer, on the unpacked values
#pragma unroll
                    for (int k = 0; k < K; ++k)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) r[k][e] = relu_(r[k][e]);
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if constexpr (!RELU_IN_PER_J) E::unpack(pre[k], r[k]);
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
            // the whole tile is scaled, rounded and packed first, into registers of its own, and only then stored -- no pack
            // writes a register that a store issued just before it still reads (fused16.hpp)
            u32x4 packed[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const factors_t av = factors(la, k);
#pragma unroll
                for (int e = 0; e < VEC; ++e) r[k][e] = av[e] * r[k][e];
                if constexpr (!LAYER) packed[k] = E::pack(r[k]);      // nothing follows the a multiply: packed chunk by chunk
            }
            if constexpr (LAYER) {
                if (has_bias) {                              // a float32 rounding of its own behind the a multiply
                    const float *const lh = lbias + (size_t)j * D;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const factors_t hv = factors(lh, k);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) r[k][e] = r[k][e] + hv[e];
                    }
                }
                if (relu_out) {                              // the activation BEHIND the layer, applied before the one rounding
#pragma unroll
                    for (int k = 0; k < K; ++k)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) r[k][e] = relu_(r[k][e]);
                }
#pragma unroll
                for (int k = 0; k < K; ++k) packed[k] = E::pack(r[k]);
            }
            __builtin_amdgcn_sched_barrier(0);
            // Segment j's first chunk of the row.  One value (J D < 2^32), shifted in 32 bits for the segment test and in 64 bits
            // for the plain kernels' addresses, as each family did before the body was shared: the registers follow the form.
            const uint32_t colq0 = j << SH;
            const size_t seg = LAYER ? (size_t)colq0 : (size_t)j << SH;
            if (!LAYER || colq0 + CPR <= n_colq) {           // (wave-uniform) a whole segment: one run of stores
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (row_ok(k)) st16<NT>(dst + out[k] + seg, packed[k]);
            } else {                                         // the narrowed last segment: chunks from n_cols on are not stored
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (row_ok(k) && colq0 + colq(k) < n_colq) st16<NT>(dst + out[k] + seg, packed[k]);
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

// ---- the four kernels: float32 / 16-bit storage, without / with the epilogue.  Each is its dynamic LDS array and the body.
template <typename T, int LOG2D, int K, bool NT>
__global__ void __launch_bounds__(256)
fused_shs_stacked_kernel(u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, const float *__restrict__ a,
                         const float *__restrict__ b, const float *__restrict__ c, uint32_t J, uint32_t n_samples, uint32_t stride,
                         uint32_t slab_rows, uint32_t n_slabs, uint32_t src_shared)
{
    static_assert(std::is_same<T, float>::value, "float32 storage");
    extern __shared__ __attribute__((aligned(16))) float fused_stacked_lds[];
    fused_stacked_fwd<T, LOG2D, K, NT, false>(fused_stacked_lds, dst, src, a, b, c, nullptr, J, n_samples, stride, slab_rows, n_slabs,
                                              src_shared, 0u, 0u, 0u);
}

template <typename T, int LOG2D, int K, bool NT>
__global__ void __launch_bounds__(256)
fused_stacked16_kernel(u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, const float *__restrict__ a,
                       const float *__restrict__ b, const float *__restrict__ c, uint32_t J, uint32_t n_samples, uint32_t stride,
                       uint32_t slab_rows, uint32_t n_slabs, uint32_t src_shared)
{
    static_assert(sizeof(T) == 2, "16-bit storage");
    extern __shared__ __attribute__((aligned(16))) float fused_stacked16_lds[];
    fused_stacked_fwd<T, LOG2D, K, NT, false>(fused_stacked16_lds, dst, src, a, b, c, nullptr, J, n_samples, stride, slab_rows,
                                              n_slabs, src_shared, 0u, 0u, 0u);
}

template <typename T, int LOG2D, int K, bool NT>
__global__ void __launch_bounds__(256)
fused_shs_stacked_layer_kernel(u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, const float *__restrict__ a,
                               const float *__restrict__ b, const float *__restrict__ c, const float *__restrict__ bias, uint32_t J,
                               uint32_t n_samples, uint32_t stride, uint32_t slab_rows, uint32_t n_slabs, uint32_t src_shared,
                               uint32_t n_colq, uint32_t ld_q, uint32_t opts)
{
    static_assert(std::is_same<T, float>::value, "float32 storage");
    extern __shared__ __attribute__((aligned(16))) float fused_stacked_layer_lds[];
    fused_stacked_fwd<T, LOG2D, K, NT, true>(fused_stacked_layer_lds, dst, src, a, b, c, bias, J, n_samples, stride, slab_rows,
                                             n_slabs, src_shared, n_colq, ld_q, opts);
}

template <typename T, int LOG2D, int K, bool NT>
__global__ void __launch_bounds__(256)
fused_stacked16_layer_kernel(u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, const float *__restrict__ a,
                             const float *__restrict__ b, const float *__restrict__ c, const float *__restrict__ bias, uint32_t J,
                             uint32_t n_samples, uint32_t stride, uint32_t slab_rows, uint32_t n_slabs, uint32_t src_shared,
                             uint32_t n_colq, uint32_t ld_q, uint32_t opts)
{
    static_assert(sizeof(T) == 2, "16-bit storage");
    extern __shared__ __attribute__((aligned(16))) float fused_stacked16_layer_lds[];
    fused_stacked_fwd<T, LOG2D, K, NT, true>(fused_stacked16_layer_lds, dst, src, a, b, c, bias, J, n_samples, stride, slab_rows,
                                             n_slabs, src_shared, n_colq, ld_q, opts);
}

// ---- host side: the checks are compiled once (abi.hip); each entry's translation unit instantiates its own kernels through
// fused_stacked_fwd_run<T, LAYER>.
struct FusedStackedLayerArgs {
    void *dst;
    const void *src, *a, *b, *c, *bias;
    int64_t n_blocks, n_samples, sample_stride, n_cols, ld_dst;
    int32_t log2d;
    uint32_t opts;
    bool src_shared, nt;
    FusedBwdGeom geom;
};

// what one entry (storage type, with or without the epilogue) is called: its kernel, the prefix of its messages, the label
// of its launch
template <typename T, bool LAYER>
struct FusedStackedFwdEntry {
    static constexpr bool F32 = sizeof(T) == 4;
    static constexpr const char *kernel = LAYER ? (F32 ? "fused_shs_stacked_layer_kernel" : "fused_stacked16_layer_kernel")
                                                : (F32 ? "fused_shs_stacked_kernel" : "fused_stacked16_kernel");
    static constexpr const char *what = LAYER ? (F32 ? "whvi_fused_shs_stacked_layer" : "whvi_fused_shs_stacked_layer16")
                                              : (F32 ? "whvi_fused_shs_stacked" : "whvi_fused_shs_stacked16");
    static constexpr const char *label = LAYER ? (F32 ? "fused_shs_stacked_layer" : "fused_shs_stacked_layer (16-bit)")
                                               : (F32 ? "fused_shs_stacked" : "fused_shs_stacked (16-bit)");
};

// Every argument check of the six entries, before any device call.  what: the prefix of the entry's messages; esize: bytes of
// an activation element (a chunk is 16 / esize columns); layer: the entry has an epilogue -- without one, bias, n_cols and
// ld_dst are not looked at and r gets bias = nullptr, opts = 0, n_cols = ld_dst = J D.  WHVI_OK with launch = false: nothing to
// launch.
int fused_stacked_fwd_check(const char *what, int esize, bool layer, FusedStackedLayerArgs &r, bool &launch, void *dst,
                            const void *src, const void *a, const void *b, const void *c, const void *bias, int64_t J, int64_t S,
                            int64_t stride, int32_t log2d, int64_t n_cols, int64_t ld_dst, int32_t flags);

template <typename T, bool LAYER, int L>
inline void fused_stacked_fwd_launch_one(const FusedStackedLayerArgs &r, hipStream_t st)
{
    constexpr int VEC = Elem<T>::VEC, K = fused_bwd_k(L, VEC);
    const dim3 grid((unsigned)(r.n_samples * r.geom.n_slabs));
    const size_t lds = (size_t)r.n_blocks * (r.bias ? 4 : 3) * sizeof(float) << L;
    note_launch<T>(FusedStackedFwdEntry<T, LAYER>::kernel, L, K, r.nt);
    auto *const dst = (u32x4 *)r.dst;
    const auto *const src = (const u32x4 *)r.src;
    const auto *const a = (const float *)r.a, *const b = (const float *)r.b, *const c = (const float *)r.c;
    const uint32_t J = (uint32_t)r.n_blocks, S = (uint32_t)r.n_samples, stride = (uint32_t)r.sample_stride;
    const uint32_t slab_rows = (uint32_t)r.geom.slab_rows, n_slabs = (uint32_t)r.geom.n_slabs, shared = r.src_shared ? 1u : 0u;
    auto launch = [&](auto nt) {
        constexpr bool NT = decltype(nt)::value != 0;
        if constexpr (LAYER) {
            const auto *const bias = (const float *)r.bias;
            const uint32_t n_colq = (uint32_t)(r.n_cols / VEC), ld_q = (uint32_t)(r.ld_dst / VEC);
            if constexpr (VEC == 4)
                hipLaunchKernelGGL((fused_shs_stacked_layer_kernel<T, L, K, NT>), grid, dim3(256), lds, st, dst, src, a, b, c, bias, J,
                                   S, stride, slab_rows, n_slabs, shared, n_colq, ld_q, r.opts);
            else
                hipLaunchKernelGGL((fused_stacked16_layer_kernel<T, L, K, NT>), grid, dim3(256), lds, st, dst, src, a, b, c, bias, J,
                                   S, stride, slab_rows, n_slabs, shared, n_colq, ld_q, r.opts);
        } else if constexpr (VEC == 4) {
            hipLaunchKernelGGL((fused_shs_stacked_kernel<T, L, K, NT>), grid, dim3(256), lds, st, dst, src, a, b, c, J, S, stride,
                               slab_rows, n_slabs, shared);
        } else {
            hipLaunchKernelGGL((fused_stacked16_kernel<T, L, K, NT>), grid, dim3(256), lds, st, dst, src, a, b, c, J, S, stride,
                               slab_rows, n_slabs, shared);
        }
    };
    if (r.nt) launch(IC<1>{});
    else launch(IC<0>{});
}

template <typename T, bool LAYER>
inline int fused_stacked_fwd_run(void *dst, const void *src, const void *a, const void *b, const void *c, const void *bias,
                                 int64_t n_blocks, int64_t n_samples, int64_t sample_stride, int32_t log2d, int64_t n_cols,
                                 int64_t ld_dst, int32_t flags, void *stream)
{
    using Entry = FusedStackedFwdEntry<T, LAYER>;
    FusedStackedLayerArgs r;
    bool launch = false;
    const int rc = fused_stacked_fwd_check(Entry::what, (int)sizeof(T), LAYER, r, launch, dst, src, a, b, c, bias, n_blocks, n_samples,
                                           sample_stride, log2d, n_cols, ld_dst, flags);
    if (rc != WHVI_OK || !launch) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (log2d) {
    case 6: fused_stacked_fwd_launch_one<T, LAYER, 6>(r, st); break;
    case 7: fused_stacked_fwd_launch_one<T, LAYER, 7>(r, st); break;
    case 8: fused_stacked_fwd_launch_one<T, LAYER, 8>(r, st); break;
    case 9: fused_stacked_fwd_launch_one<T, LAYER, 9>(r, st); break;
    case 10: fused_stacked_fwd_launch_one<T, LAYER, 10>(r, st); break;
    default: fused_stacked_fwd_launch_one<T, LAYER, 11>(r, st); break;
    }
    return after_launch(Entry::label);
}

}  // namespace whvi
