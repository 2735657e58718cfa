#pragma once
// whvi_amd/csrc/fused_stacked.hpp -- the rectangular fastfood layer: J independent square operators applied to the SAME rows,
// their outputs written side by side, in ONE launch.  ABI: include/whvi_hip.h (whvi_fused_shs_stacked_f32).
//
//     dst[r, j D + n] = a[j, n] * H(b[j, s(r), :] (.) H(c[j, :] (.) src[r, :]))[n],       j = 0 .. J - 1
//
// i.e. block j of the (rows, J D) output is whvi_fused_shs_f32(src, a[j], b[j], c[j], axis = COL) -- the paper's stacking of
// square S1 H diag(g) H S2 blocks (src/weights.py: WHVIStackedMatrix.setup_dimensions) -- without J launches that each read the
// row again and a concatenation that reads and writes all of it once more: a row is read once and J segments are written,
// (1 + J) D elements per row instead of about 4 J D.
//
// Arithmetic: every multiply is its own rounding and the two transforms are fwht_tile with fused_shs_kernel's template
// arguments and sign sequence (0 -> SIGN_MID -> 0), exactly as fused_bwd.hpp issues them (fused_bwd_fwht): segment j has, element
// for element, the value of the per-block launch (the sign of an exact zero exempt, as for that entry).
//
// Geometry: fused_shs_bwd_kernel's.  A block of four waves owns (sample s, a slab of that sample's rows) -- fused_bwd_geom, a
// function of the arguments alone -- stages all J triples a_j, b_{j,s}, c_j in LDS once (12 D J bytes) and walks its slab one
// wave tile at a time, in fused_shs_kernel's chunk layout (chunk k * 64 + lane): one row for D >= 1024, 1024 / D rows below.
// Per tile the input is loaded once and kept in registers; for each j it is copied, run through scale -> transform -> scale ->
// transform -> scale, the whole output tile is packed, and only then stored: D-wide segments at column offset j D, row pitch
// J D.  No atomics, no scratch, no allocation, no synchronisation.
#include "dispatch.hpp"
#include "fused_bwd.hpp"

namespace whvi {

constexpr int FUSED_STACKED_MIN_LOG2D = 6, FUSED_STACKED_MAX_LOG2D = 11;
constexpr int64_t FUSED_STACKED_LDS_BYTES = 65536;        // whvi_mlp_apply_supported's budget
inline bool fused_stacked_supported(int log2d, int64_t n_blocks)
{
    if (log2d < FUSED_STACKED_MIN_LOG2D || log2d > FUSED_STACKED_MAX_LOG2D || n_blocks < 1) return false;
    return n_blocks <= FUSED_STACKED_LDS_BYTES / ((int64_t)12 << log2d);
}

// dst : (n_samples * stride, J D).  src : the same rows of D, or (stride, D) with src_shared (row r of every sample reads
// src[r]).  a, c : (J, D); b : (J, n_samples, D).  LDS: J triples [a_j | b_{j,s} | c_j] of D floats.
// NT: the streamed accesses (the stores, and the loads of a source of its own) take the non-temporal policy.
template <typename T, int LOG2D, int K, bool NT>
__global__ void __launch_bounds__(256)
fused_shs_stacked_kernel(u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, const float *__restrict__ a,
                         const float *__restrict__ b, const float *__restrict__ c, uint32_t J, uint32_t n_samples, uint32_t stride,
                         uint32_t slab_rows, uint32_t n_slabs, uint32_t src_shared)
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
    extern __shared__ __attribute__((aligned(16))) float fused_stacked_lds[];

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t r_begin = slab * slab_rows;
    const uint32_t r_end = (uint64_t)r_begin + slab_rows < stride ? r_begin + slab_rows : stride;
    constexpr uint32_t QUADS = (uint32_t)D / 4;
    for (uint32_t j = 0; j < J; ++j) {
        f4 *const la = reinterpret_cast<f4 *>(fused_stacked_lds + (size_t)3 * j * D);
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
            const f4 *const la = reinterpret_cast<const f4 *>(fused_stacked_lds + (size_t)3 * j * D);
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
            // the whole tile is scaled and packed first, into registers of its own, and only then stored
            u32x4 packed[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const f4 av = la[colq(k)];
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

// ---- host side
struct FusedStackedArgs {
    void *dst;
    const void *src, *a, *b, *c;
    int64_t n_blocks, n_samples, sample_stride;
    int32_t log2d;
    bool src_shared, nt;
    FusedBwdGeom geom;
};

template <typename T, int L>
inline void fused_stacked_launch_one(const FusedStackedArgs &r, hipStream_t st)
{
    constexpr int K = fused_bwd_k(L, Elem<T>::VEC);
    const dim3 grid((unsigned)(r.n_samples * r.geom.n_slabs));
    const size_t lds = (size_t)r.n_blocks * 3 * sizeof(float) << L;
    note_launch<T>("fused_shs_stacked_kernel", L, K, r.nt);
#define WHVI_FUSED_STACKED(NT)                                                                                          \
    hipLaunchKernelGGL((fused_shs_stacked_kernel<T, L, K, NT>), grid, dim3(256), lds, st, (u32x4 *)r.dst, (const u32x4 *)r.src, \
                       (const float *)r.a, (const float *)r.b, (const float *)r.c, (uint32_t)r.n_blocks, (uint32_t)r.n_samples, \
                       (uint32_t)r.sample_stride, (uint32_t)r.geom.slab_rows, (uint32_t)r.geom.n_slabs, r.src_shared ? 1u : 0u)
    if (r.nt) WHVI_FUSED_STACKED(true);
    else WHVI_FUSED_STACKED(false);
#undef WHVI_FUSED_STACKED
}

}  // namespace whvi
