#pragma once
// whvi_amd/csrc/fused_stacked16.hpp -- the rectangular fastfood layer in ONE launch for 16-bit ACTIVATION storage (__half /
// __hip_bfloat16) with float32 scale vectors.  ABI: include/whvi_hip.h (whvi_fused_shs_stacked_f16 / _bf16).
//
//     dst[r, j D + n] = pack(a[j, n] * H(b[j, s(r), :] (.) H(c[j, :] (.) unpack(src[r, :])))[n]),       j = 0 .. J - 1
//
// A sibling of fused_shs_stacked_kernel (fused_stacked.hpp), not another instantiation of it: that template's symbols are
// pinned, it takes float32 storage only, and a chunk of 16-bit storage holds 8 elements whose float32 factors are two reads.
//
// Contract (fused16.hpp's): Elem<T>::unpack in, every multiply its own float32 rounding, float32 butterflies in the forward's
// sign sequence (0 -> SIGN_MID -> 0, fused_bwd_fwht with VEC = 8 -- the chain fused_shs_bwd_kernel<__half> runs for grad_x), ONE
// Elem<T>::pack when an element is stored, nothing rounded to 16 bits in between: block j of the (rows, J D) output is, element
// for element, whvi_fused_shs_ex_f16 / _bf16(src, a[j], b[j], c[j], axis = COL) (the sign of an exact zero exempt, as for that
// entry) -- with a shared source, that launch on the expanded source.
//
// Geometry: fused_shs_stacked_kernel's with 8-element chunks.  A block of four waves owns (sample s, a slab of that sample's
// rows) -- fused_bwd_geom -- stages all J triples a_j, b_{j,s}, c_j in LDS once (float32: 12 D J bytes) in fused16.hpp's split
// layout (the first halves of all chunks, then the second halves: both 16-byte reads of a chunk's eight factors are
// lane-contiguous) and walks its slab one wave tile at a time: K = fused_bwd_k(LOG2D, 8) chunks per lane, one row for
// D >= 1024, 1024 / D rows below.  Per tile the input is loaded once and kept packed in registers; for each j it is unpacked,
// run through scale -> transform -> scale -> transform -> scale, the whole output tile is packed, and only then stored: D-wide
// segments at column offset j D, row pitch J D.  No atomics, no scratch, no allocation, no synchronisation.
#include "dispatch.hpp"
#include "fused_bwd.hpp"
#include "fused_stacked.hpp"

namespace whvi {

// the float32 launch's rule: the staged vectors are float32 whatever the activations are stored in
inline bool fused_stacked16_supported(int log2d, int64_t n_blocks) { return fused_stacked_supported(log2d, n_blocks); }

// dst : (n_samples * stride, J D) of T.  src : the same rows of D, or (stride, D) with src_shared (row r of every sample reads
// src[r]).  a, c : (J, D) float32; b : (J, n_samples, D) float32.  LDS: J triples [a_j | b_{j,s} | c_j] of D floats, each vector
// in the split layout.
// NT: the streamed accesses (the stores, and the loads of a source of its own) take the non-temporal policy.
template <typename T, int LOG2D, int K, bool NT>
__global__ void __launch_bounds__(256)
fused_stacked16_kernel(u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, const float *__restrict__ a,
                       const float *__restrict__ b, const float *__restrict__ c, uint32_t J, uint32_t n_samples, uint32_t stride,
                       uint32_t slab_rows, uint32_t n_slabs, uint32_t src_shared)
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
    extern __shared__ __attribute__((aligned(16))) float fused_stacked16_lds[];

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t r_begin = slab * slab_rows;
    const uint32_t r_end = (uint64_t)r_begin + slab_rows < stride ? r_begin + slab_rows : stride;
    // piece i of a vector (16 bytes) is half (i & 1) of chunk i >> 1: it goes to piece (i & 1) * QUADS / 2 + (i >> 1)
    constexpr uint32_t QUADS = (uint32_t)D / 4;
    for (uint32_t j = 0; j < J; ++j) {
        f4 *const la = reinterpret_cast<f4 *>(fused_stacked16_lds + (size_t)3 * j * D);
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
    // the eight factors of the lane's chunk k of a staged vector
    auto factors = [&](const float *v, int k) __attribute__((always_inline)) -> factors_t {
        factors_t f;
        f.q[0] = reinterpret_cast<const f4 *>(v)[colq(k)];
        f.q[1] = reinterpret_cast<const f4 *>(v + D / 2)[colq(k)];
        return f;
    };
    const size_t sample_row0 = (size_t)s * stride;
    const size_t src_row0 = src_shared ? 0 : sample_row0;
    const size_t pitch = (size_t)J << SH;                   // chunks of one output row

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
        for (int k = 0; k < K; ++k) out[k] = (sample_row0 + rt + row_in(k)) * pitch + colq(k);
#pragma unroll 1
        for (uint32_t j = 0; j < J; ++j) {
            const float *const la = fused_stacked16_lds + (size_t)3 * j * D;
            const float *const lb = la + D, *const lc = lb + D;
            float r[K][VEC];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                E::unpack(pre[k], r[k]);
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
                packed[k] = E::pack(r[k]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (row_ok(k)) st16<NT>(dst + out[k] + ((size_t)j << SH), packed[k]);
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
// through fused_stacked16_run<T>.

// Every argument check of whvi_fused_shs_stacked_f16 / _bf16, before any device call (whvi_fused_shs_stacked_f32's, in its
// order, with 2-byte activations).  WHVI_OK with launch = false: nothing to launch.
int fused_stacked16_check(FusedStackedArgs &r, bool &launch, void *dst, const void *src, const void *a, const void *b,
                          const void *c, int64_t J, int64_t S, int64_t stride, int32_t log2d, int32_t flags);

template <typename T, int L>
inline void fused_stacked16_launch_one(const FusedStackedArgs &r, hipStream_t st)
{
    constexpr int K = fused_bwd_k(L, Elem<T>::VEC);
    const dim3 grid((unsigned)(r.n_samples * r.geom.n_slabs));
    const size_t lds = (size_t)r.n_blocks * 3 * sizeof(float) << L;
    note_launch<T>("fused_stacked16_kernel", L, K, r.nt);
#define WHVI_FUSED_STACKED16(NT)                                                                                        \
    hipLaunchKernelGGL((fused_stacked16_kernel<T, L, K, NT>), grid, dim3(256), lds, st, (u32x4 *)r.dst, (const u32x4 *)r.src, \
                       (const float *)r.a, (const float *)r.b, (const float *)r.c, (uint32_t)r.n_blocks, (uint32_t)r.n_samples, \
                       (uint32_t)r.sample_stride, (uint32_t)r.geom.slab_rows, (uint32_t)r.geom.n_slabs, r.src_shared ? 1u : 0u)
    if (r.nt) WHVI_FUSED_STACKED16(true);
    else WHVI_FUSED_STACKED16(false);
#undef WHVI_FUSED_STACKED16
}

template <typename T>
inline int fused_stacked16_run(void *dst, const void *src, const void *a, const void *b, const void *c, int64_t n_blocks,
                               int64_t n_samples, int64_t sample_stride, int32_t log2d, int32_t flags, void *stream)
{
    FusedStackedArgs r;
    bool launch = false;
    const int rc = fused_stacked16_check(r, launch, dst, src, a, b, c, n_blocks, n_samples, sample_stride, log2d, flags);
    if (rc != WHVI_OK || !launch) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (log2d) {
    case 6: fused_stacked16_launch_one<T, 6>(r, st); break;
    case 7: fused_stacked16_launch_one<T, 7>(r, st); break;
    case 8: fused_stacked16_launch_one<T, 8>(r, st); break;
    case 9: fused_stacked16_launch_one<T, 9>(r, st); break;
    case 10: fused_stacked16_launch_one<T, 10>(r, st); break;
    default: fused_stacked16_launch_one<T, 11>(r, st); break;
    }
    return after_launch("fused_shs_stacked (16-bit)");
}

}  // namespace whvi
