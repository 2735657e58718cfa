#pragma once
// whvi_amd/csrc/diag_apply_stacked.hpp -- the batched pass of a reference-mode WHVIStackedMatrix (src/weights.py:111-208) of any
// width WITHOUT its matrices: all J diagonal blocks of every Monte-Carlo sample written by one launch.
//
// The stacked weight is J square blocks on top of each other, each exactly D * diag(s1[j] (.) u[j] (.) s2[j]) as written
// (diag_apply.hpp, SURVEY.md finding 1), so `x_padded @ W.T` is, per block, one product per output added to exact zeros:
//
//     out[s, b, j D + i] = relu?( relu?(x[(s,) b, i]) * w[j, s, i] + 0 (+ bias[j D + i]) )      j D + i < n_cols
//     w[j, s, :] = wbar_diag(s1[j], s2[j], u[j, 0]) + wbar_diag(s1[j], s2[j], u[j, 1 + s])
//
// with diag_apply_kernel's arithmetic per block -- diag_w_chunk / wbar_diag as they are (same roundings, same NaN rule for
// non-finite parameters), the accumulator's + 0, relu_ (NaN passes) -- and its row poison applied to every block: a
// non-finite entry of a row at column k, tested after relu_in, turns the outputs i != k of that row into NaN in EVERY block (in
// the dense product it meets the exact zeros of every block's rows), output k of each block stays the plain product.
// Bit-identical to whvi_diag_apply per block + cat + narrowing (tests/test_stacked_diag_gpu.py).
//
// Geometry: a block owns (sample s, a slab of batch rows), like small_k_apply_kernel and mlp_apply_kernel.  It stages that
// sample's J diagonals (and the bias) in LDS once -- 4 J D (8 J D with a bias) bytes, at most 64 KiB -- then each wave walks
// row groups: a row's 16-byte chunks are loaded ONCE (rows shorter than 256 floats go several to a wave, MlpGeom's lane
// groups), counted for the poison behind a wave ballot, and then the wave walks j, multiplying and storing.  The launch reads
// every input row once and writes n_cols floats per row: a write stream.  No atomics, no scratch.
//
// The kernels are instantiated per C = chunks per lane and row (1 for D <= 256, D / 256 beyond) rather than per log2(D): the
// row length reaches wbar_diag as a compile-time constant through a switch in the (cold) staging loop only.
#include "dispatch.hpp"
#include "diag_apply.hpp"

namespace whvi {

constexpr int64_t STACKED_DIAG_MAX_LDS = (int64_t)64 * 1024;
constexpr uint32_t STACKED_OPT_X_SHARED = 32u, STACKED_OPT_VEC = 64u, STACKED_OPT_WIDE = 128u;      // next to DIAG_OPT_*: one option word

// one sample's J diagonals and the bias (counted whether there is one or not: the rule must not depend on the call)
constexpr int64_t stacked_diag_lds_bytes(int log2d, int64_t n_blocks) { return ((int64_t)8 << log2d) * n_blocks; }

inline bool stacked_diag_supported(int log2d, int64_t n_blocks)
{
    return log2d >= 2 && log2d <= 12 && n_blocks >= 1 && n_blocks <= STACKED_DIAG_MAX_LDS &&
           stacked_diag_lds_bytes(log2d, n_blocks) <= STACKED_DIAG_MAX_LDS;
}

constexpr int stacked_diag_c(int log2d) { return log2d <= 8 ? 1 : 1 << (log2d - 8); }      // chunks per lane and row
template <int C> struct StackedDiagGeom {
    static constexpr int R = C >= 4 ? 1 : 4 / C;          // rows per lane group and iteration: four 16-byte loads in flight
};

// x : (S B, D) or (B, D); s1, s2 : (J, D); u : (J, U, D), U = S + (opts & DIAG_OPT_MEAN); bias : J D floats or null;
// out : S B rows at pitch ld_out, n_cols columns of each written.  C = stacked_diag_c(log2d).
template <typename T, int C, bool NT>      // (T = float; named so that whvi_last_kernel prints the real symbol)
__global__ void __launch_bounds__(256)
diag_apply_stacked_kernel(float *__restrict__ out, const float *__restrict__ x, const float *__restrict__ s1,
                          const float *__restrict__ s2, const float *__restrict__ u, const float *__restrict__ bias, uint32_t S,
                          uint32_t B, uint32_t J, uint32_t log2d, uint32_t n_cols, int64_t ld_out, uint32_t opts,
                          uint32_t slab_rows, uint32_t n_slabs)
{
    constexpr int R = StackedDiagGeom<C>::R;
    typedef float f4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float stacked_lds[];
    const uint32_t cpr = 1u << (log2d - 2);                // 16-byte chunks per row
    const uint32_t n_chunks = J << (log2d - 2);            // ... of the J blocks
    float *lw = stacked_lds, *lb = stacked_lds + (size_t)n_chunks * 4;
    const uint32_t mean_plus = opts & DIAG_OPT_MEAN;
    const bool relu_in = (opts & DIAG_OPT_RELU_IN) != 0, relu_out = (opts & DIAG_OPT_RELU_OUT) != 0;
    const bool shared = (opts & STACKED_OPT_X_SHARED) != 0, vec = (opts & STACKED_OPT_VEC) != 0;
    const bool has_bias = bias != nullptr;

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t b0 = slab * slab_rows, b1 = b0 + slab_rows < B ? b0 + slab_rows : B;

    // ---- this sample's diagonals (and the bias) into LDS: chunk q of block j at float 4 (j cpr + q)
    {
        const size_t U = (size_t)S + mean_plus;
        for (uint32_t idx = threadIdx.x; idx < n_chunks; idx += 256) {
            const uint32_t j = idx >> (log2d - 2), q = idx & (cpr - 1);
            const float *a = s1 + ((size_t)j << log2d), *c = s2 + ((size_t)j << log2d), *uj = u + ((j * U) << log2d);
            float wv[4] = {0.f, 0.f, 0.f, 0.f};
            switch (log2d) {
#define WHVI_STACKED_W(L) case L: diag_w_chunk<float, L>(a, c, uj, s, mean_plus, q * 4, wv); break;
                WHVI_STACKED_W(2) WHVI_STACKED_W(3) WHVI_STACKED_W(4) WHVI_STACKED_W(5) WHVI_STACKED_W(6) WHVI_STACKED_W(7)
                WHVI_STACKED_W(8) WHVI_STACKED_W(9) WHVI_STACKED_W(10) WHVI_STACKED_W(11) WHVI_STACKED_W(12)
#undef WHVI_STACKED_W
            default: break;
            }
            reinterpret_cast<f4 *>(lw)[idx] = f4{wv[0], wv[1], wv[2], wv[3]};
            if (has_bias) reinterpret_cast<f4 *>(lb)[idx] = reinterpret_cast<const f4 *>(bias)[idx];
        }
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // lanes per row: the whole wave from D = 256 on, cpr lanes below (64 / cpr rows side by side)
    const uint32_t lsh = C == 1 ? log2d - 2 : 6u;
    const uint32_t lanes = 1u << lsh;
    const uint32_t grp = (uint32_t)lane >> lsh, col = (uint32_t)lane & (lanes - 1);
    // short rows (D < 256), 64 / lanes lane groups per wave: the groups hold different ROWS and each walks all blocks -- or, with
    // at least as many blocks as groups (STACKED_OPT_WIDE), all hold the SAME rows and group g takes blocks g, g + G, ..., so that
    // one store instruction writes 1 KiB of one output row instead of 64 / lanes pieces of as many rows
    const bool wide = (opts & STACKED_OPT_WIDE) != 0;
    const uint32_t row_grp = wide ? 0u : grp, j0 = wide ? grp : 0u, jstep = wide ? 64u >> lsh : 1u;
    const uint32_t rpi = (wide ? 1u : 64u >> lsh) * R;     // rows per wave iteration
    const size_t orow0 = (size_t)s * B;
    for (uint32_t rb = b0 + wave * rpi; rb < b1; rb += 4 * rpi) {
        const uint32_t r0 = rb + row_grp * R;              // rows r0 .. r0 + R - 1 (past b1: a valid row's operands, never stored)
        float h[R][C][4];
        bool bad = false;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t row = r0 + r < b1 ? r0 + r : b1 - 1;
            const f4 *xr = reinterpret_cast<const f4 *>(x + (((shared ? (size_t)0 : orow0) + row) << log2d));
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const f4 v = xr[col + k * 64];
#pragma unroll
                for (int e = 0; e < 4; ++e) h[r][k][e] = v[e];
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < C; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (relu_in) h[r][k][e] = relu_(h[r][k][e]);      // the activation in FRONT of this layer, applied on load
                    bad |= !__builtin_isfinite(h[r][k][e]);
                }
        if (__builtin_amdgcn_ballot_w64(bad) != 0) {
            // (rare) diag_apply_kernel's row poison: every OTHER element of a row that holds a non-finite value becomes NaN
#pragma unroll
            for (int r = 0; r < R; ++r) {
                uint32_t cnt = 0;
#pragma unroll
                for (int k = 0; k < C; ++k)
#pragma unroll
                    for (int e = 0; e < 4; ++e) cnt += __builtin_isfinite(h[r][k][e]) ? 0u : 1u;
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) {
                    const uint32_t o = (uint32_t)__shfl_xor((int)cnt, m, 64);
                    if ((uint32_t)m < lanes) cnt += o;                 // the lanes of the row
                }
#pragma unroll
                for (int k = 0; k < C; ++k)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (cnt - (__builtin_isfinite(h[r][k][e]) ? 0u : 1u) != 0u) h[r][k][e] = __builtin_nan("");
            }
        }
        // ---- the wave walks the blocks: one product per output, + 0, + bias, the activation behind, the store
        for (uint32_t j = j0; (j << log2d) < n_cols; j += jstep) {
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const uint32_t q = j * cpr + col + k * 64;             // chunk of the output row
                const uint32_t oc = q * 4;                             // its first column
                if (oc >= n_cols) continue;
                const f4 wc = reinterpret_cast<const f4 *>(lw)[q];
                f4 bc = f4{0.f, 0.f, 0.f, 0.f};
                if (has_bias) bc = reinterpret_cast<const f4 *>(lb)[q];
                const bool whole = vec && oc + 4 <= n_cols;           // 16-byte store: aligned pitch and base, a whole chunk
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        // the one non-zero product of the dot product + the +0 the block's other D - 1 products (exact zeros)
                        // sum to in a GEMM's accumulator: a product of -0 comes out as +0 like there
                        v[e] = h[r][k][e] * wc[e] + 0.0f;
                        if (has_bias) v[e] = v[e] + bc[e];
                        if (relu_out) v[e] = relu_(v[e]);
                    }
                    if (r0 + r < b1) {
                        float *p = out + (orow0 + r0 + r) * (size_t)ld_out + oc;
                        if (whole) {
                            st16<NT>(reinterpret_cast<u32x4 *>(p), Elem<float>::pack(v));
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (oc + e < n_cols) p[e] = v[e];
                        }
                    }
                }
            }
        }
    }
}

// The launch of one call, from stacked_diag_check
struct StackedDiagLaunch {
    dim3 grid;
    size_t lds;
    uint32_t slab_rows, n_slabs, opts;
    bool nt;
};

constexpr int32_t STACKED_DIAG_FLAGS = WHVI_DIAG_X_SHARED | WHVI_DIAG_MEAN_PLUS | WHVI_DIAG_RELU_IN | WHVI_DIAG_RELU_OUT |
                                       WHVI_DIAG_TUNE_NT | WHVI_DIAG_TUNE_CACHED;

// Every argument check of whvi_diag_apply_stacked_f32, before any launch.  WHVI_OK with ln.grid.x = 0: nothing to launch.
inline int stacked_diag_check(StackedDiagLaunch &ln, const void *out, const void *x, const void *s1, const void *s2, const void *u,
                              const void *bias, int64_t S, int64_t B, int32_t log2d, int64_t J, int64_t n_cols, int64_t ld_out,
                              int32_t flags)
{
    ln.grid = dim3(0);
    if (S < 0 || B < 0 || J < 0 || n_cols < 0 || ld_out < 0)
        return fail(WHVI_ERR_ARG, "whvi_diag_apply_stacked: negative size%s", "");
    if (flags & ~STACKED_DIAG_FLAGS) return fail(WHVI_ERR_ARG, "whvi_diag_apply_stacked: unknown flags%s 0x%llx", "", flags);
    if (log2d < 2 || log2d > 12)
        return fail(WHVI_ERR_SIZE, "whvi_diag_apply_stacked: log2(D)%s = %lld is outside the supported range [2, 12]", "", log2d);
    if (!stacked_diag_supported(log2d, J))
        return fail(WHVI_ERR_SIZE, "whvi_diag_apply_stacked: n_blocks%s = %lld: one sample's diagonals and bias need 8 J D bytes "
                    "of LDS, 1 <= J and 64 KiB at most", "", J);
    const int64_t D = (int64_t)1 << log2d;
    if (n_cols < 1 || n_cols > J * D)
        return fail(WHVI_ERR_ARG, "whvi_diag_apply_stacked: n_cols%s = %lld is outside [1, J D = %lld]", "", n_cols, J * D);
    if (ld_out < n_cols || ld_out >= ((int64_t)1 << 31))
        return fail(WHVI_ERR_ARG, "whvi_diag_apply_stacked: ld_out%s = %lld is below n_cols = %lld (or beyond 2^31)", "", ld_out, n_cols);
    if (S == 0 || B == 0) return WHVI_OK;
    if (S >= ((int64_t)1 << 32) || B >= ((int64_t)1 << 31) || S * B >= ((int64_t)1 << 32))      // (B: the row loop's stride must not wrap)
        return fail(WHVI_ERR_SIZE, "whvi_diag_apply_stacked: rows are indexed with 32 bits%s", "");
    const int64_t rows = S * B;
    if (!out || !x || !s1 || !s2 || !u) return fail(WHVI_ERR_ARG, "whvi_diag_apply_stacked: null pointer%s", "");
    if ((((uintptr_t)x | (uintptr_t)s1 | (uintptr_t)s2 | (uintptr_t)u | (uintptr_t)bias) & 15) || ((uintptr_t)out & 3))
        return fail(WHVI_ERR_ALIGN, "whvi_diag_apply_stacked: an input pointer%s is not 16-byte aligned (or out not 4-byte)", "");
    const bool shared = (flags & WHVI_DIAG_X_SHARED) != 0, mean = (flags & WHVI_DIAG_MEAN_PLUS) != 0;
    {
        const struct { const void *p; int64_t n; } in[] = {
            {x, (shared ? B : rows) * D}, {s1, J * D}, {s2, J * D}, {u, J * (S + (mean ? 1 : 0)) * D}, {bias, J * D}};
        const char *op = (const char *)out, *oe = op + ((rows - 1) * ld_out + n_cols) * 4;
        for (const auto &t : in) {
            const char *p = (const char *)t.p;
            if (p != nullptr && p < oe && op < p + t.n * 4)
                return fail(WHVI_ERR_OVERLAP, "whvi_diag_apply_stacked: out overlaps an input%s (in-place use included)", "");
        }
    }
    // slabs: about four blocks per CU over all samples, every wave of a block with at least one row group
    const int c = stacked_diag_c(log2d);
    const int64_t groups = c == 1 ? (int64_t)256 >> log2d : 1;      // lane groups per wave (rows shorter than 256 floats)
    const bool wide = groups > 1 && J >= groups;                    // the groups share their rows and split the blocks (kernel)
    const int64_t rpi = (wide ? 1 : groups) * (c >= 4 ? 1 : 4 / c);      // the kernel's rows per wave iteration
    int64_t n_slabs = (4 * (int64_t)num_cu() + S - 1) / S;
    const int64_t most = (B + 4 * rpi - 1) / (4 * rpi);
    if (n_slabs > most) n_slabs = most;
    if (n_slabs < 1) n_slabs = 1;
    const int64_t slab_rows = (B + n_slabs - 1) / n_slabs;
    n_slabs = (B + slab_rows - 1) / slab_rows;
    if (n_slabs * S >= ((int64_t)1 << 31)) return fail(WHVI_ERR_SIZE, "whvi_diag_apply_stacked: too many blocks%s", "");
    ln.lds = (size_t)(stacked_diag_lds_bytes(log2d, J) / (bias != nullptr ? 1 : 2));
    ln.grid = dim3((unsigned)(n_slabs * S));
    ln.slab_rows = (uint32_t)slab_rows;
    ln.n_slabs = (uint32_t)n_slabs;
    // 16-byte stores where every chunk of every row is aligned: base and pitch (dword stores otherwise, and for a ragged chunk)
    const bool vec = ((uintptr_t)out & 15) == 0 && (ld_out & 3) == 0;
    ln.opts = (mean ? DIAG_OPT_MEAN : 0u) | ((flags & WHVI_DIAG_RELU_IN) ? DIAG_OPT_RELU_IN : 0u) |
              ((flags & WHVI_DIAG_RELU_OUT) ? DIAG_OPT_RELU_OUT : 0u) | (shared ? STACKED_OPT_X_SHARED : 0u) | (vec ? STACKED_OPT_VEC : 0u) |
              (wide ? STACKED_OPT_WIDE : 0u);
    // a write stream: non-temporal stores once the bytes written exceed the Infinity Cache (the input is read once, or shared)
    ln.nt = (flags & WHVI_DIAG_TUNE_NT) ? true : (flags & WHVI_DIAG_TUNE_CACHED) ? false : rows * n_cols * 4 > NT_MIN_BYTES;
    return WHVI_OK;
}

}  // namespace whvi
