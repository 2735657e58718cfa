#pragma once
// whvi_amd/csrc/diag_apply_stacked_bwd.hpp -- backward of diag_apply_stacked.hpp's launch in one call: the closed form of
//
//     out[s, b, j D + i] = relu?( relu?(x[(s,) b, i]) * w[j, s, i] + 0 (+ bias[j D + i]) )      j D + i < n_cols
//
// on the n_cols columns that were written.  With gm = g masked by the output activation (the pre-activation recomputed from
// x, the diagonal and the bias with the forward's roundings, as diag_apply_bwd_kernel does):
//
//     grad_x[s, b, i]  = [relu_in: x > 0] * sum_{j : j D + i < n_cols} gm[s, b, j D + i] * w[j, s, i]      ascending j
//     gw[j, s, i]      = sum_b gm[s, b, j D + i] * relu?(x[(s,) b, i])          gb[j, s, i] = sum_b gm[s, b, j D + i]
//
// and diag_apply_bwd_finish_kernel's chain from gw to (dL/du, dL/ds1, dL/ds2) per block.
//
// Geometry: diag_apply_bwd_kernel's layout on the g-ROW.  A block owns (sample s, a slab of batch rows).  A thread owns CPT
// 16-byte chunks of the J D-wide row (chunk q = c TPR + tcol: block j = q / (D / 4), column chunk q mod (D / 4) of x), TPR =
// min(J D / 4, 256) threads cover a row and RG = 256 / TPR rows are in flight per step, UNR steps per iteration.  The thread
// computes its diagonal chunks ONCE into registers (the cold switch over log2(D) keeps the instantiations per chunk count) and
// keeps sum_b gm x and sum_b gm in registers: J D <= 8192 is at most 8 chunks per thread.  Chunks from n_cols on are never
// read -- neither g nor the x columns under them (WHVILinear(1024, 2): one chunk of each 4 KiB row of x).
// grad_x needs the sum over the threads that share a column: with more than one written block the products of the rows in
// flight go through an LDS tile and are added in ascending j; one written block (every n -> 2 output layer) stores directly.
// The whole grad_x row is written (+0 where no written column reaches).  part: (S, n_slabs, 2, C) = {sum g x, sum g} with
// C = n_cols rounded up to a chunk -- the written columns only, so an n -> 2 layer's workspace is 8 floats per slab; the
// finishing launch adds the slabs in slab order (four-way, like diag_apply_bwd_finish_kernel).  No atomics, no scratch.
#include "dispatch.hpp"
#include "diag_apply.hpp"
#include "diag_apply_stacked.hpp"

namespace whvi {

constexpr int64_t STACKED_DIAG_BWD_MAX_COLS = 8192;      // J D: eight 16-byte chunks per thread at most

inline bool stacked_diag_bwd_supported(int log2d, int64_t n_blocks)
{
    return log2d >= 2 && log2d <= 12 && n_blocks >= 1 && n_blocks <= STACKED_DIAG_BWD_MAX_COLS &&
           (n_blocks << log2d) <= STACKED_DIAG_BWD_MAX_COLS;
}

// chunks per thread for a row of nc = J D / 4 chunks
constexpr int stacked_diag_bwd_cpt(int64_t nc) { return nc <= 256 ? 1 : nc <= 512 ? 2 : nc <= 1024 ? 4 : 8; }
template <int CPT> struct StackedDiagBwdGeom {
    static constexpr int UNR = CPT >= 4 ? 1 : 4 / CPT;      // row steps per iteration: four 16-byte loads of g in flight
};
constexpr int stacked_diag_bwd_unr(int cpt) { return cpt >= 4 ? 1 : 4 / cpt; }
// rows a block has in flight per step: 256 / TPR
constexpr int64_t stacked_diag_bwd_rg(int64_t nc) { return nc < 256 ? 256 / nc : 1; }

template <typename T, int CPT, bool NT, bool WANT_GX>      // (T = float; named so that whvi_last_kernel prints the real symbol)
__global__ void __launch_bounds__(256)
stacked_diag_bwd_kernel(float *__restrict__ gx, float *__restrict__ part, const float *__restrict__ g, const float *__restrict__ x,
                        const float *__restrict__ s1, const float *__restrict__ s2, const float *__restrict__ u,
                        const float *__restrict__ bias, uint32_t S, uint32_t B, uint32_t J, uint32_t log2d, uint32_t n_cols,
                        int64_t ld_g, uint32_t opts, uint32_t slab_rows, uint32_t n_slabs)
{
    constexpr int UNR = StackedDiagBwdGeom<CPT>::UNR;
    typedef float f4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float sdb_lds[];
    const uint32_t mean_plus = opts & DIAG_OPT_MEAN;
    const bool relu_in = (opts & DIAG_OPT_RELU_IN) != 0, relu_out = (opts & DIAG_OPT_RELU_OUT) != 0;
    const bool shared = (opts & STACKED_OPT_X_SHARED) != 0, vec = (opts & STACKED_OPT_VEC) != 0;
    const bool has_bias = bias != nullptr;
    const uint32_t cpr = 1u << (log2d - 2);                // 16-byte chunks per row of x
    const uint32_t nc = J << (log2d - 2);                  // ... of the J D-wide row
    const uint32_t tpr = CPT == 1 ? nc : 256u;             // threads per row (CPT == 1: nc <= 256)
    const uint32_t rgs = 256u / tpr;                       // rows in flight per step
    const uint32_t tcol = threadIdx.x % tpr, rg = threadIdx.x / tpr;
    const bool lane_on = rg < rgs;                         // (256 mod tpr threads have no row)
    const uint32_t live_chunks = (n_cols + 3u) >> 2;       // chunks that hold a written column
    const bool xchg = WANT_GX && n_cols > (1u << log2d);   // more than one written block: grad_x is a sum over threads

    const uint32_t s = blockIdx.x / n_slabs, slab = blockIdx.x - s * n_slabs;
    const uint32_t b0 = slab * slab_rows, b1 = b0 + slab_rows < B ? b0 + slab_rows : B;

    // ---- this thread's chunks: the diagonal (and the bias) once, into registers
    uint32_t q[CPT], xc[CPT], nlive[CPT];                  // chunk of the row, its chunk of x, its written columns (0 .. 4)
    float w[CPT][4], bv[CPT][4], acc[CPT][4], accb[CPT][4];
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
        q[c] = (uint32_t)c * tpr + tcol;
        xc[c] = q[c] & (cpr - 1);
        nlive[c] = (lane_on && q[c] < live_chunks) ? (n_cols - q[c] * 4u < 4u ? n_cols - q[c] * 4u : 4u) : 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[c][e] = bv[c][e] = acc[c][e] = accb[c][e] = 0.f;
        if (nlive[c] != 0u) {
            const uint32_t j = q[c] >> (log2d - 2);
            const size_t U = (size_t)S + mean_plus;
            const float *a = s1 + ((size_t)j << log2d), *cc = s2 + ((size_t)j << log2d), *uj = u + ((j * U) << log2d);
            switch (log2d) {
#define WHVI_STACKED_W(L) case L: diag_w_chunk<float, L>(a, cc, uj, s, mean_plus, xc[c] * 4, w[c]); break;
                WHVI_STACKED_W(2) WHVI_STACKED_W(3) WHVI_STACKED_W(4) WHVI_STACKED_W(5) WHVI_STACKED_W(6) WHVI_STACKED_W(7)
                WHVI_STACKED_W(8) WHVI_STACKED_W(9) WHVI_STACKED_W(10) WHVI_STACKED_W(11) WHVI_STACKED_W(12)
#undef WHVI_STACKED_W
            default: break;
            }
            if (has_bias && relu_out) {
                const f4 bc = reinterpret_cast<const f4 *>(bias)[q[c]];
#pragma unroll
                for (int e = 0; e < 4; ++e) bv[c][e] = bc[e];
            }
        }
    }

    const size_t orow0 = (size_t)s * B;
    const size_t xrow0 = shared ? (size_t)0 : orow0;
    for (uint32_t rb = b0; rb < b1; rb += rgs * UNR) {      // (uniform trip count: the exchange has barriers inside)
        u32x4 rgv[UNR][CPT], rxv[UNR][CPT];
#pragma unroll
        for (int i = 0; i < UNR; ++i) {
            const uint32_t row = rb + (uint32_t)i * rgs + rg;
#pragma unroll
            for (int c = 0; c < CPT; ++c) {
                rgv[i][c] = rxv[i][c] = u32x4{0u, 0u, 0u, 0u};
                if (row < b1 && nlive[c] != 0u) {
                    const float *gp = g + (orow0 + row) * (size_t)ld_g + (size_t)q[c] * 4;
                    if (vec && nlive[c] == 4u) {
                        rgv[i][c] = *reinterpret_cast<const u32x4 *>(gp);
                    } else {                               // another pitch, or the ragged last chunk: dword loads
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if ((uint32_t)e < nlive[c]) rgv[i][c][e] = __float_as_uint(gp[e]);
                    }
                    rxv[i][c] = *reinterpret_cast<const u32x4 *>(x + ((xrow0 + row) << log2d) + (size_t)xc[c] * 4);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < UNR; ++i) {
            const uint32_t rl = (uint32_t)i * rgs + rg;    // row of the step's tile
            const uint32_t row = rb + rl;
            const bool ok = lane_on && row < b1;
#pragma unroll
            for (int c = 0; c < CPT; ++c) {
                float gv[4], xr[4], xv[4], o[4];
                Elem<float>::unpack(rgv[i][c], gv);
                Elem<float>::unpack(rxv[i][c], xr);
#pragma unroll
                for (int e = 0; e < 4; ++e) xv[e] = relu_in ? relu_(xr[e]) : xr[e];
                if (relu_out) {
                    // the fused activation's backward: the forward's pre-activation recomputed with its roundings; the gradient
                    // passes unless the activation's result is <= 0 (so it passes on a NaN, torch's threshold_backward)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float z = xv[e] * w[c][e] + 0.0f;
                        if (has_bias) z = z + bv[c][e];
                        if (relu_(z) <= 0.f) gv[e] = 0.f;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool on = ok && (uint32_t)e < nlive[c];
                    if (on) {
                        acc[c][e] = acc[c][e] + gv[e] * xv[e];
                        accb[c][e] = accb[c][e] + gv[e];
                    }
                    o[e] = gv[e] * w[c][e];
                    if (relu_in && xv[e] <= 0.f) o[e] = 0.f;
                    if (!on) o[e] = 0.f;
                }
                if constexpr (WANT_GX) {
                    if (xchg) {
                        if (ok && nlive[c] != 0u)
                            reinterpret_cast<f4 *>(sdb_lds)[(size_t)rl * nc + q[c]] = f4{o[0], o[1], o[2], o[3]};
                    } else if (ok && q[c] < cpr) {         // one written block: its thread stores, +0 beyond n_cols
                        st16<NT>(reinterpret_cast<u32x4 *>(gx + ((orow0 + row) << log2d)) + q[c], Elem<float>::pack(o));
                    }
                }
            }
        }
        if constexpr (WANT_GX) {
            if (xchg) {
                __syncthreads();
                // the step's rows x the chunks of x: products of the blocks that reach the chunk, added in ascending j
                const uint32_t n_out = (rgs * UNR) << (log2d - 2);
                for (uint32_t idx = threadIdx.x; idx < n_out; idx += 256) {
                    const uint32_t rl = idx >> (log2d - 2), k = idx & (cpr - 1), row = rb + rl;
                    if (row >= b1) continue;
                    const f4 *t = reinterpret_cast<const f4 *>(sdb_lds) + (size_t)rl * nc;
                    f4 sum = t[k];
                    for (uint32_t qq = cpr + k; qq < live_chunks; qq += cpr) {
                        const f4 p = t[qq];
#pragma unroll
                        for (int e = 0; e < 4; ++e) sum[e] = sum[e] + p[e];
                    }
                    float v[4] = {sum[0], sum[1], sum[2], sum[3]};
                    st16<NT>(reinterpret_cast<u32x4 *>(gx + ((orow0 + row) << log2d)) + k, Elem<float>::pack(v));
                }
                __syncthreads();
            }
        }
    }

    const size_t LC = (size_t)live_chunks * 4;             // the written columns, rounded up to a chunk
    float *p0 = part + ((size_t)s * n_slabs + slab) * 2 * LC;
    if (CPT == 1 && rgs > 1) {
        // row groups -> one sum per column, in group order
        f4 *red = reinterpret_cast<f4 *>(sdb_lds);
        red[threadIdx.x] = f4{acc[0][0], acc[0][1], acc[0][2], acc[0][3]};
        red[256 + threadIdx.x] = f4{accb[0][0], accb[0][1], accb[0][2], accb[0][3]};
        __syncthreads();
        if (rg == 0 && tcol < live_chunks) {
            f4 a = red[tcol], b = red[256 + tcol];
            for (uint32_t r = 1; r < rgs; ++r) {
                const f4 pa = red[r * tpr + tcol], pb = red[256 + r * tpr + tcol];
#pragma unroll
                for (int e = 0; e < 4; ++e) { a[e] = a[e] + pa[e]; b[e] = b[e] + pb[e]; }
            }
            reinterpret_cast<f4 *>(p0)[tcol] = a;
            reinterpret_cast<f4 *>(p0 + LC)[tcol] = b;
        }
    } else {
#pragma unroll
        for (int c = 0; c < CPT; ++c)
            if (lane_on && q[c] < live_chunks) {
                reinterpret_cast<f4 *>(p0)[q[c]] = f4{acc[c][0], acc[c][1], acc[c][2], acc[c][3]};
                reinterpret_cast<f4 *>(p0 + LC)[q[c]] = f4{accb[c][0], accb[c][1], accb[c][2], accb[c][3]};
            }
    }
}

// out: (4, J, U, D), U = mean_plus + S: diag_apply_bwd_finish_kernel's (4, U, D) per block, zeros from column n_cols on
template <typename T>
__global__ void __launch_bounds__(256)
stacked_diag_bwd_finish_kernel(T *__restrict__ out, const T *__restrict__ part, const T *__restrict__ s1, const T *__restrict__ s2,
                               const T *__restrict__ u, uint32_t n_slabs, uint32_t log2d, uint32_t J, uint32_t S, uint32_t n_cols,
                               uint32_t mean_plus)
{
    const uint32_t col = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    const uint32_t D = 1u << log2d, JD = J << log2d;
    if (col >= JD) return;
    const uint32_t j = col >> log2d, i = col & (D - 1);
    const uint32_t U = mean_plus + S;
    const size_t o = ((size_t)j * U + mean_plus + k) * D + i, slot = (size_t)J * U * D;
    if (col >= n_cols) {
        out[o] = out[slot + o] = out[2 * slot + o] = out[3 * slot + o] = (T)0;
        return;
    }
    const size_t LC = (size_t)((n_cols + 3u) & ~3u);       // part: (S, n_slabs, 2, LC)
    const T *p = part + (size_t)k * n_slabs * 2 * LC + col;
    T gw[4] = {0, 0, 0, 0}, gb[4] = {0, 0, 0, 0};
    uint32_t sl = 0;
    for (; sl + 4 <= n_slabs; sl += 4)
#pragma unroll
        for (int q = 0; q < 4; ++q) { gw[q] = gw[q] + p[(size_t)(sl + q) * 2 * LC]; gb[q] = gb[q] + p[(size_t)(sl + q) * 2 * LC + LC]; }
    for (int q = 0; sl < n_slabs; ++sl, ++q) { gw[q] = gw[q] + p[(size_t)sl * 2 * LC]; gb[q] = gb[q] + p[(size_t)sl * 2 * LC + LC]; }
    const T w = (gw[0] + gw[1]) + (gw[2] + gw[3]), bsum = (gb[0] + gb[1]) + (gb[2] + gb[3]);
    const T Dd = (T)D, a = s1[col], c = s2[col];
    const T *uj = u + (size_t)j * U * D;
    const T uk = uj[(size_t)(mean_plus + k) * D + i], u0 = mean_plus ? uj[i] : (T)0;
    out[o] = w * (a * Dd * c);
    out[slot + o] = w * (mean_plus ? Dd * (u0 * c) + Dd * (uk * c) : Dd * (uk * c));
    out[2 * slot + o] = w * (a * Dd * (mean_plus ? u0 + uk : uk));
    out[3 * slot + o] = bsum;
}

// whvi_diag_apply_stacked_bwd_slabs: about eight blocks per CU over all samples, at least four iterations of rows per block
inline int64_t stacked_diag_bwd_slabs(int64_t S, int64_t B, int32_t log2d, int64_t J)
{
    if (S < 1 || B < 1 || !stacked_diag_bwd_supported(log2d, J)) return 1;
    const int64_t nc = J << (log2d - 2);
    const int64_t rows = stacked_diag_bwd_rg(nc) * stacked_diag_bwd_unr(stacked_diag_bwd_cpt(nc));      // rows per iteration
    const int64_t want = (8 * (int64_t)num_cu() + S - 1) / S;
    const int64_t most = (B + rows * 4 - 1) / (rows * 4);
    int64_t n = want < most ? want : most;
    if (n < 1) n = 1;
    const int64_t slab_rows = (B + n - 1) / n;
    return (B + slab_rows - 1) / slab_rows;
}

struct StackedDiagBwdLaunch {
    dim3 grid;
    size_t lds;
    uint32_t slab_rows, opts;
    bool nt;
};

// Every argument check of whvi_diag_apply_stacked_bwd_f32, before any launch.  WHVI_OK with ln.grid.x = 0: nothing to launch.
inline int stacked_diag_bwd_check(StackedDiagBwdLaunch &ln, const void *grad_x, const void *out, const void *part, const void *g,
                                  const void *x, const void *s1, const void *s2, const void *u, const void *bias, int64_t S,
                                  int64_t B, int32_t log2d, int64_t J, int64_t n_cols, int64_t ld_g, int64_t n_slabs, int32_t flags)
{
    ln.grid = dim3(0);
    if (S < 0 || B < 0 || J < 0 || n_cols < 0 || ld_g < 0 || n_slabs < 0)
        return fail(WHVI_ERR_ARG, "whvi_diag_apply_stacked_bwd: negative size%s", "");
    if (flags & ~STACKED_DIAG_FLAGS) return fail(WHVI_ERR_ARG, "whvi_diag_apply_stacked_bwd: unknown flags%s 0x%llx", "", flags);
    if (log2d < 2 || log2d > 12)
        return fail(WHVI_ERR_SIZE, "whvi_diag_apply_stacked_bwd: log2(D)%s = %lld is outside the supported range [2, 12]", "", log2d);
    if (!stacked_diag_bwd_supported(log2d, J))
        return fail(WHVI_ERR_SIZE, "whvi_diag_apply_stacked_bwd: n_blocks%s = %lld: a row of J D columns, 1 <= J and J D <= 8192", "", J);
    const int64_t D = (int64_t)1 << log2d;
    if (n_cols < 1 || n_cols > J * D)
        return fail(WHVI_ERR_ARG, "whvi_diag_apply_stacked_bwd: n_cols%s = %lld is outside [1, J D = %lld]", "", n_cols, J * D);
    if (ld_g < n_cols || ld_g >= ((int64_t)1 << 31))
        return fail(WHVI_ERR_ARG, "whvi_diag_apply_stacked_bwd: ld_g%s = %lld is below n_cols = %lld (or beyond 2^31)", "", ld_g, n_cols);
    if (S == 0 || B == 0) return WHVI_OK;
    if (S >= ((int64_t)1 << 32) || B >= ((int64_t)1 << 31) || S * B >= ((int64_t)1 << 32))
        return fail(WHVI_ERR_SIZE, "whvi_diag_apply_stacked_bwd: rows are indexed with 32 bits%s", "");
    const int64_t rows = S * B;
    if (!out || !part || !g || !x || !s1 || !s2 || !u) return fail(WHVI_ERR_ARG, "whvi_diag_apply_stacked_bwd: null pointer%s", "");
    if ((((uintptr_t)grad_x | (uintptr_t)out | (uintptr_t)part | (uintptr_t)x | (uintptr_t)s1 | (uintptr_t)s2 | (uintptr_t)u |
          (uintptr_t)bias) & 15) || ((uintptr_t)g & 3))
        return fail(WHVI_ERR_ALIGN, "whvi_diag_apply_stacked_bwd: a pointer%s is not 16-byte aligned (or g not 4-byte)", "");
    if (n_slabs < 1 || n_slabs > B)
        return fail(WHVI_ERR_ARG, "whvi_diag_apply_stacked_bwd: bad slab count%s (B = %lld, n_slabs = %lld)", "", B, n_slabs);
    const int64_t slab_rows = (B + n_slabs - 1) / n_slabs;
    if ((B + slab_rows - 1) / slab_rows != n_slabs)
        return fail(WHVI_ERR_ARG, "whvi_diag_apply_stacked_bwd: n_slabs%s = %lld is not a slab count of this batch (use "
                    "whvi_diag_apply_stacked_bwd_slabs)", "", n_slabs);
    if (n_slabs * S >= ((int64_t)1 << 31) || S > 65535)      // (S: the finishing launch's second grid dimension)
        return fail(WHVI_ERR_SIZE, "whvi_diag_apply_stacked_bwd: too many blocks%s (65535 samples at most)", "");
    const bool shared = (flags & WHVI_DIAG_X_SHARED) != 0, mean = (flags & WHVI_DIAG_MEAN_PLUS) != 0;
    const int64_t U = S + (mean ? 1 : 0);
    {
        const struct { const void *p; int64_t n; } in[] = {{g, (rows - 1) * ld_g + n_cols}, {x, (shared ? B : rows) * D},
            {s1, J * D}, {s2, J * D}, {u, J * U * D}, {bias, J * D}};
        const struct { const void *p; int64_t n; } res[] = {{grad_x, rows * D}, {out, 4 * J * U * D}, {part, S * n_slabs * 2 * ((n_cols + 3) / 4 * 4)}};
        for (const auto &r : res) {
            const char *op = (const char *)r.p, *oe = op + r.n * 4;
            if (op == nullptr) continue;
            for (const auto &t : in) {
                const char *p = (const char *)t.p;
                if (p != nullptr && p < oe && op < p + t.n * 4)
                    return fail(WHVI_ERR_OVERLAP, "whvi_diag_apply_stacked_bwd: grad_x, out or part%s overlaps an input", "");
            }
        }
    }
    const int64_t nc = J << (log2d - 2);
    const int cpt = stacked_diag_bwd_cpt(nc);
    const int64_t rg = stacked_diag_bwd_rg(nc);
    const bool xchg = grad_x != nullptr && n_cols > D;
    // the exchange tile of the rows in flight (every chunk of the row), or the row groups' partial sums
    const int64_t tile = xchg ? rg * stacked_diag_bwd_unr(cpt) * nc * 16 : 0, red = rg > 1 ? 2 * 256 * 16 : 0;
    ln.lds = (size_t)(tile > red ? tile : red);
    ln.grid = dim3((unsigned)(n_slabs * S));
    ln.slab_rows = (uint32_t)slab_rows;
    // 16-byte loads of g where every chunk of every row is aligned: base and pitch (dword loads otherwise, and for a ragged chunk)
    const bool vec = ((uintptr_t)g & 15) == 0 && (ld_g & 3) == 0;
    ln.opts = (mean ? DIAG_OPT_MEAN : 0u) | ((flags & WHVI_DIAG_RELU_IN) ? DIAG_OPT_RELU_IN : 0u) |
              ((flags & WHVI_DIAG_RELU_OUT) ? DIAG_OPT_RELU_OUT : 0u) | (shared ? STACKED_OPT_X_SHARED : 0u) | (vec ? STACKED_OPT_VEC : 0u);
    // grad_x is the launch's write stream: non-temporal stores by the forward's rule, on the bytes written
    ln.nt = grad_x != nullptr && ((flags & WHVI_DIAG_TUNE_NT) ? true : (flags & WHVI_DIAG_TUNE_CACHED) ? false : rows * D * 4 > NT_MIN_BYTES);
    return WHVI_OK;
}

}  // namespace whvi
