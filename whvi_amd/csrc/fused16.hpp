#pragma once
// whvi_amd/csrc/fused16.hpp -- the fused scale -> FWHT -> scale -> FWHT -> scale pipeline for 16-bit ACTIVATION storage
// (__half / __hip_bfloat16) with float32 scale vectors.  C ABI: whvi_fused_shs_ex_f16 / _bf16 (include/whvi_hip.h).
//
// A sibling of fused_shs_kernel (kernels.hpp) rather than another instantiation of it: that template takes its scale
// vectors in the storage type and its symbols are pinned (tests/test_build.py, profiles/hbm_traffic.json), so its
// parameter list stays as it is and the mixed-type case gets its own, much smaller, template -- column axis with a source
// only, no identity input, no shared source, no one-transform form.
//
// Contract: Elem<T>::unpack in, every multiply its own f32 rounding (-ffp-contract=off), f32 butterflies in the reference's
// ascending stage order, ONE Elem<T>::pack (RNE) when the tile is stored -- i.e. the f32 pipeline on the exactly-upcast
// input, rounded once.  Nothing is rounded to 16 bits in between.
//
// Layout: a 16-byte chunk holds 8 elements, a tile is 64 * K chunks per wave (K = 8: 8 KiB and 64 accumulator registers
// per lane for D <= 4096; K = 16: one row of 8192, 128 registers).  The eight f32 scale factors of a chunk are two 16-byte
// loads: from LDS when the block stages the vector (split layout: the first halves of all chunks, then the second halves, so
// that either read is lane-contiguous), from L2 otherwise.
#include "kernels.hpp"

namespace whvi {

// 16-byte load of four f32 scale factors at (wave-uniform base) + lane * 32 + byte offset: the two halves of the lane's chunk
__device__ __forceinline__ u32x4 uniform_ld16_pitch32(const void *base, uint32_t bytes, int lane, int byte_offset)
{
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * 32, byte_offset, 0));
}

// POLICY: POLICY_DPP = the signed DPP / permlane network of the f32 fused kernel for both transforms, the one value that is
// instantiated.  (Tried: fwht_tile_lds for both -- one private 16.6 KB slab per wave caps a CU at 8 waves, and at 4 once
// vectors are staged beside the slabs at D >= 2048 -- DESIGN.md 5.2b.)
template <typename T, int LOG2D, int K, bool NT, int POLICY, int STAGE, int BLOCK = 256>
__global__ void __launch_bounds__(BLOCK)
fused_shs16_kernel(u32x4 *dst, const u32x4 *src, const float *a, const float *b, const float *c,
                   int64_t n_chunks, int64_t n_tiles, FastDiv by_sample_stride, FastDiv by_n_samples, int flags)
{
    using E = Elem<T>;
    using A = typename E::acc;
    constexpr int VEC = E::VEC;
    constexpr int LV = ilog2(VEC);
    constexpr int TILE = 64 * K;
    constexpr int SH = LOG2D - LV;           // log2(chunks per row)
    constexpr uint32_t CPR = 1u << SH;
    constexpr int D = 1 << LOG2D;
    static_assert(sizeof(T) == 2 && VEC == 8 && sizeof(A) == 4, "16-bit storage, f32 arithmetic");
    static_assert(LOG2D >= LV && LOG2D <= LV + 6 + ilog2(K), "rows of one chunk up to one tile");
    static_assert(STAGE == STAGE_NONE || SH >= 6, "staging: rows of at least 64 chunks");
    static_assert(POLICY == POLICY_DPP, "the DPP / permlane network is the only form of this kernel");
    const bool a_per_sample = flags & WHVI_FUSED_A_PER_SAMPLE;
    const bool c_per_sample = flags & WHVI_FUSED_C_PER_SAMPLE;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // streams: XCD-contiguous block order and a block barrier before the stores, as in fused_shs_kernel
    int64_t blk = blockIdx.x;
    if (NT && (gridDim.x & 7) == 0) blk = (blk & 7) * (int64_t)(gridDim.x >> 3) + (blk >> 3);
    const int64_t t = blk * (BLOCK / 64) + wave;
    const bool active = t < n_tiles;                          // wave-uniform; a block always has at least one active wave
    const int64_t base = t * TILE;
    const uint32_t row0 = (uint32_t)(base >> SH);             // first row of the tile (wave-uniform)
    auto sample_index = [&](uint32_t row) __attribute__((always_inline)) -> uint32_t {
        return by_n_samples.mod(by_sample_stride.div(row));
    };

    // ---- request order as in fused_shs_kernel: the block's scale vectors first, the tile right behind them; the vectors
    // are written to LDS and the block barrier passes while the tile's loads are still in flight
    extern __shared__ __attribute__((aligned(16))) char whvi_smem[];
    constexpr int NSTAGED = STAGE == STAGE_ABC ? 3 : (STAGE == STAGE_AC ? 2 : 0);
    A *const lds_a = reinterpret_cast<A *>(whvi_smem);
    A *const lds_c = lds_a + D;
    A *const lds_b = lds_c + D;
    typedef A quad_t __attribute__((ext_vector_type(4)));
    constexpr int QUADS = D / 4;                                      // 16-byte pieces of one vector
    constexpr int STG_ITERS = (QUADS + BLOCK - 1) / BLOCK;
    quad_t stg[NSTAGED > 0 ? NSTAGED : 1][STG_ITERS];
    const A *stg_src[3] = {nullptr, nullptr, nullptr};                // c, a, b (the order they are needed in)
    A *const stg_dst[3] = {lds_c, lds_a, lds_b};
    if constexpr (STAGE != STAGE_NONE) {
        // the block's sample: read only where a vector is per-sample (all rows of the block then share it: host-checked)
        const uint32_t blk_row0 = (uint32_t)((blk * (BLOCK / 64) * TILE) >> SH);
        const size_t s_off = (size_t)sample_index(blk_row0) << LOG2D;
        stg_src[0] = c == nullptr ? nullptr : c + (c_per_sample ? s_off : 0);
        stg_src[1] = a == nullptr ? nullptr : a + (a_per_sample ? s_off : 0);
        stg_src[2] = (STAGE == STAGE_ABC && b != nullptr) ? b + s_off : nullptr;
#pragma unroll
        for (int v = 0; v < NSTAGED; ++v)
            if (stg_src[v] != nullptr) {
#pragma unroll
                for (int j = 0; j < STG_ITERS; ++j) {
                    const int q = threadIdx.x + j * BLOCK;
                    if (q < QUADS) stg[v][j] = *reinterpret_cast<const quad_t *>(stg_src[v] + q * 4);
                }
            }
        __builtin_amdgcn_sched_barrier(0);
    }
    // the tile: chunks of a partial last tile beyond the buffer read as zero and are never written, waves past the last
    // tile touch nothing.  Full 64-register tiles take plain global loads behind a wave-uniform branch (kernels.hpp)
    const uint32_t tile_bytes = active ? (uint32_t)((n_chunks - base < TILE ? n_chunks - base : (int64_t)TILE) * 16) : 0u;
    u32x4 raw[K];
    if (K <= 8 && tile_bytes == TILE * 16) {
#pragma unroll
        for (int k = 0; k < K; ++k) raw[k] = ld16<NT>(src + base + k * 64 + lane);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) raw[k] = uniform_ld16<NT>(src + base, tile_bytes, lane, k * 1024);
    }
    if constexpr (STAGE != STAGE_NONE) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int v = 0; v < NSTAGED; ++v)
            if (stg_src[v] != nullptr) {
#pragma unroll
                for (int j = 0; j < STG_ITERS; ++j) {
                    const int q = threadIdx.x + j * BLOCK;          // piece q = half (q & 1) of chunk q >> 1
                    if (q < QUADS) *reinterpret_cast<quad_t *>(stg_dst[v] + (q & 1) * (D / 2) + (q >> 1) * 4) = stg[v][j];
                }
            }
        __syncthreads();
    }
    if (!active) {
        if constexpr (NT) __syncthreads();      // the store-alignment barrier below
        return;
    }

    constexpr int SIGN_MID = fwht_sign_out<VEC, LOG2D>(0);
    static_assert(fwht_sign_out<VEC, LOG2D>(SIGN_MID) == 0, "two transforms restore the sign convention");
    auto transform = [&](A (&r)[K][VEC], auto second) {
        fwht_tile<A, VEC, K, LOG2D, POLICY_DPP, FUSED_PKMASK, true, decltype(second)::value ? SIGN_MID : 0>(r, lane);
    };

    // rows never straddle tiles; rows of >= 64 chunks (UNIFORM): the row of k-step k -- hence its sample and its vector's
    // base -- is wave-uniform
    constexpr bool UNIFORM = SH >= 6;
    constexpr int KPR = UNIFORM ? (int)CPR / 64 : 1;                   // k-steps per row
    auto chunk_col = [&](int k) __attribute__((always_inline)) -> uint32_t { return (uint32_t)(k * 64 + lane) & (CPR - 1); };
    // the eight factors of chunk k from L2
    auto scale = [&](const A *vec, bool per_sample, int k, A (&out)[VEC]) __attribute__((always_inline)) {
        u32x4 lo, hi;
        if constexpr (UNIFORM) {
            const uint32_t keep = per_sample ? 0xFFFFFFFFu : 0u;
            const A *p = vec + ((size_t)(sample_index(row0 + (uint32_t)(k / KPR)) & keep) << LOG2D);
            lo = uniform_ld16_pitch32(p, (uint32_t)sizeof(A) << LOG2D, lane, (k % KPR) * 2048);
            hi = uniform_ld16_pitch32(p, (uint32_t)sizeof(A) << LOG2D, lane, (k % KPR) * 2048 + 16);
        } else {
            const uint32_t row = row0 + (uint32_t)((k * 64 + lane) >> SH);
            const uint32_t vec_base = per_sample ? sample_index(row) << LOG2D : 0u;
            const u32x4 *p = reinterpret_cast<const u32x4 *>(vec + (size_t)vec_base + chunk_col(k) * VEC);
            lo = p[0];
            hi = p[1];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t l = lo[e], h = hi[e];
            out[e] = __uint_as_float(l);
            out[4 + e] = __uint_as_float(h);
        }
    };

    A r[K][VEC];

    // vectors staged in LDS: multiplied straight out of LDS, four chunks (eight 16-byte reads) in flight at a time
    auto apply_staged = [&](const A *staged) __attribute__((always_inline)) {
        constexpr int G = 4;
#pragma unroll
        for (int k0 = 0; k0 < K; k0 += G) {
            quad_t lo[G], hi[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                lo[g] = *reinterpret_cast<const quad_t *>(staged + chunk_col(k0 + g) * 4);
                hi[g] = *reinterpret_cast<const quad_t *>(staged + D / 2 + chunk_col(k0 + g) * 4);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    r[k0 + g][e] = lo[g][e] * r[k0 + g][e];
                    r[k0 + g][4 + e] = hi[g][e] * r[k0 + g][4 + e];
                }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // vectors from L2: five eighths of the chunks requested up front, the rest once as many have been multiplied in
    // (64 + 40 registers instead of 64 + 64 next to the tile, as in fused_shs_kernel)
    constexpr int UPFRONT = (K * 5) / 8;
    constexpr int LATE = K - UPFRONT;
    auto scale_chunkwise = [&](const A *vec, bool per_sample) __attribute__((always_inline)) {
        A v[K][VEC];
#pragma unroll
        for (int k = 0; k < UPFRONT; ++k) scale(vec, per_sample, k, v[k]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < LATE; ++k)
#pragma unroll
            for (int e = 0; e < VEC; ++e) r[k][e] = v[k][e] * r[k][e];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = UPFRONT; k < K; ++k) scale(vec, per_sample, k, v[k]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = LATE; k < K; ++k)
#pragma unroll
            for (int e = 0; e < VEC; ++e) r[k][e] = v[k][e] * r[k][e];
    };

#pragma unroll
    for (int k = 0; k < K; ++k) E::unpack(raw[k], r[k]);
    if (c != nullptr) {
        if constexpr (STAGE != STAGE_NONE) apply_staged(lds_c);
        else scale_chunkwise(c, c_per_sample);
    }
    transform(r, IC<0>{});
    if (b != nullptr) {
        if constexpr (STAGE == STAGE_ABC) apply_staged(lds_b);
        else scale_chunkwise(b, true);
    }
    transform(r, IC<1>{});
    if (a != nullptr) {
        if constexpr (STAGE != STAGE_NONE) apply_staged(lds_a);
        else scale_chunkwise(a, a_per_sample);
    }
    // the whole tile is rounded and packed FIRST, into registers of its own, and only then stored: no pack may write a
    // register a store issued just before it still reads (tools/shipped_isa.py: store_data_hazards), and nothing but the
    // issue spacing stands between the stores
    u32x4 packed[K];
#pragma unroll
    for (int k = 0; k < K; ++k) packed[k] = E::pack(r[k]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (NT) __syncthreads();          // the block's 4 waves write their 32 KiB back together
#pragma unroll
    for (int k = 0; k < K; ++k) {
        uniform_st16<NT>(dst + base, tile_bytes, lane, k * 1024, packed[k]);
        if constexpr (NT) asm volatile("s_nop 0");                  // streaming stores never back to back (kernels.hpp)
    }
}

}  // namespace whvi
