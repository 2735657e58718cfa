/*
 * include/whvi_hip.h -- C ABI of libwhvi_hip.so, the MI355X (gfx950) replacement for the
 * reference's native FWHT module.
 *
 * Drop-in boundary.  The reference binds ONE native entry point for this path:
 *
 *     at::Tensor fwht(at::Tensor X)            src/fwht/cuda/fwht_cuda.cpp:5-14,16-18
 *       -> fwht_cuda_frontend(X)               src/fwht/cuda/fwht_cuda_kernel.cu:156-181
 *          -> fwht_batch1_kernel / _batch2_    src/fwht/cuda/fwht_cuda_kernel.cu:35-146
 *
 * exported from a Python module named `fwht_cuda` (imported at src/fwht/cuda/fwht.py:2).
 * whvi_fwht_<dtype>() below is what that binding calls instead of fwht_cuda_frontend; the
 * Python shim `fwht_cuda.py` at the repo root re-creates the module on top of it (see
 * INTEGRATION.md).  The fused entry points replace the chains of ATen ops in
 * src/weights.py:73,84,92-93 (matmul_diag_left . fwht . matmul_diag_left . fwht).
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch types.  All buffers are caller-owned DEVICE
 *     pointers, 16-byte aligned, contiguous row-major (rows, 1 << log2d).  No ownership
 *     transfer, no allocation, no host synchronisation, no global mutable state other than
 *     a thread-local error string: safe to call from several host threads (the autograd
 *     engine calls backward from its own thread) and capturable in a hipGraph.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).
 *   - the kernel launches on the device that is current for the calling thread; the
 *     Python shim sets it from the tensor (the reference never does: fwht_cuda_kernel.cu:156).
 *   - dst == src is allowed everywhere (in-place); partial overlap is not.
 *   - return value 0 = launched; negative = WHVI_ERR_*; whvi_last_error() describes it.
 *     Unlike the reference (no cudaGetLastError, silent no-op for D < 4 or D > 4096,
 *     SURVEY.md 2a) every unsupported shape is an error and launch failures are reported.
 *
 * Transform definition: unnormalised Walsh-Hadamard transform in natural (Sylvester)
 * order of every row, y = x . H_D, computed as the radix-2 butterfly network in ASCENDING
 * stride order (h = 1, 2, 4, ...) with plain add/sub -- the order of src/fwht/cpp/fwht.cpp:7-18,
 * so f32/f64 results of whvi_fwht_<dtype> are bit-identical to that reference (sign of zero included, at every size) and
 * integer results are exact.  Two opt-in forms trade the sign of a ZERO result for speed and say so where they are declared:
 * whvi_fwht_ex with WHVI_FWHT_SIGNED_LANES, and the fused pipelines whvi_fused_shs_* (a result that is -0 in the reference's
 * arithmetic may come back as +0; every other bit, NaN positions included, is the reference's).
 */
#ifndef WHVI_HIP_H
#define WHVI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WHVI_HIP_ABI_VERSION 1

/* error codes */
#define WHVI_OK               0
#define WHVI_ERR_ARG         -1   /* null pointer, negative size, bad enum            */
#define WHVI_ERR_SIZE        -2   /* log2d outside [0, whvi_max_log2d(dtype)]          */
#define WHVI_ERR_ALIGN       -3   /* a pointer is not 16-byte aligned                  */
#define WHVI_ERR_LAUNCH      -4   /* hipGetLastError() after the launch was not success*/
#define WHVI_ERR_OVERLAP     -5   /* dst and src overlap without being equal           */

/* dtype enum used by the *_ex entry point and whvi_max_log2d */
#define WHVI_F32   0
#define WHVI_F64   1
#define WHVI_F16   2   /* IEEE half storage, f32 arithmetic, one rounding on store     */
#define WHVI_I32   3   /* two's complement, wraps like the reference's int tensors     */
#define WHVI_BF16  4   /* bfloat16 storage, f32 arithmetic, one rounding on store      */

int         whvi_hip_abi_version(void);
const char *whvi_last_error(void);          /* thread-local; "" when the last call succeeded */
int         whvi_last_kernel(char *buf, int32_t size);
                                            /* writes the demangled symbol of the kernel instantiation the calling
                                             * thread's last FWHT / fused launch selected (the name rocprofv3 prints,
                                             * e.g. "whvi::fwht_rows_kernel<float, 12, 16, 0, false, true, 256, 1>");
                                             * returns its length, 0 before any launch.  Measurement aid: the
                                             * reference has no counterpart (its launcher picks between two kernels
                                             * silently, fwht_cuda_kernel.cu:156-181)                          */
int         whvi_max_log2d(int32_t dtype);  /* largest supported log2(D): 24 for f32/f64/i32 (one pass up to
                                             * D = 65536, f64 32768: a wave per row, then a block per row;
                                             * longer rows take extra high-bit passes), 16 for f16/bf16
                                             * (single pass only: one rounding)                        */

/* Measurement aid (no counterpart in the reference): a copy of `bytes` bytes (a multiple of 16; dst == src allowed) with the
 * streaming geometry of the transform kernels and no arithmetic -- one 16 KiB tile per wave, 256-thread blocks,
 * XCD-contiguous block order, non-temporal loads, block barrier, write-through non-temporal stores.  Its rate is the
 * ceiling this memory system offers the access pattern whvi_fwht_* uses; bench.py prints it as roofline.ceiling_measured. */
int whvi_stream_copy_probe(void *dst, const void *src, int64_t bytes, void *stream);

/* Batched row FWHT: dst[r, :] = FWHT(src[r, :]) for r in [0, rows).
 * Replaces fwht_cuda_frontend (fwht_cuda_kernel.cu:156-181) + the X.clone() of
 * fwht_cuda.cpp:11 (pass dst != src for the reference's out-of-place semantics).
 *
 * Sign of zero: none to mention -- these entry points run the plain add / sub butterfly network at EVERY size, so f32 / f64
 * results carry the reference's bits including the sign of a zero result (a row of negative zeros gives [-0, +0, +0, ...],
 * as -0 + -0 = -0 does in src/fwht/cpp/fwht.cpp:11-13), whatever the launch form (cache-resident, streaming, block per row).
 * The faster lane-stage form that loses that sign is opt-in: WHVI_FWHT_SIGNED_LANES of whvi_fwht_ex below. */
int whvi_fwht_f32 (void *dst, const void *src, int64_t rows, int32_t log2d, void *stream);
int whvi_fwht_f64 (void *dst, const void *src, int64_t rows, int32_t log2d, void *stream);
int whvi_fwht_f16 (void *dst, const void *src, int64_t rows, int32_t log2d, void *stream);
int whvi_fwht_bf16(void *dst, const void *src, int64_t rows, int32_t log2d, void *stream);
int whvi_fwht_i32 (void *dst, const void *src, int64_t rows, int32_t log2d, void *stream);

/* Same transform with an explicit kernel variant, for tuning and for cross-checking the
 * cross-lane code paths against each other on hardware.  variant == 0 is the production launch
 * (what whvi_fwht_<dtype> does); otherwise
 *   bits 0..2 : butterfly network / loop form
 *                 0  DPP + permlane network, persistent loop with register prefetch of the next tile
 *                 1,5  every cross-lane stage through ds_bpermute (__shfl_xor), one tile per wave
 *                 2  DPP + permlane network, one tile per wave, cached accesses
 *                 3  LDS-staged network (fwht_tile_lds), one tile per wave, cached accesses
 *                 4  as 0 with non-temporal accesses
 *                 6  as 2 with non-temporal loads and write-through non-temporal stores (production form)
 *                 7  as 3 with non-temporal accesses
 *   bits 4..5 : threads per block, 0 = 256, 1 = 512, 2 = 1024 (576 for the LDS-staged network)
 *   bits 8..19: cap of the grid in blocks per CU (0 = uncapped: one tile per wave)
 *   bits 20..22: launch form of rows LONGER than one wavefront tile (D > 8192; f64 > 4096), every dtype:
 *                 0  production (a block per row up to D = 65536, pipelined grid chosen by size; pieces + passes beyond)
 *                 1  2^12-element pieces + high-bit passes for every long row (round 1's form)
 *                 2  one row per block      3  persistent pipelined grid (where that instantiation exists)
 *                 4  as 1 with every pass over the whole buffer instead of 128 MiB row groups
 *   bit 23 (WHVI_FWHT_SIGNED_LANES), with bits 0..19 zero: the production launch of whvi_fwht_<dtype>, except that STREAMING
 *                 launches (buffers beyond the 256 MiB Infinity Cache) of f32 rows of D = 512 .. 2048 and f64 rows of
 *                 D = 64 .. 2048 run their lane stages as fused multiply-adds by +/-1 (round 2-3: +1.7 %; since round 4's store
 *                 spacing the plain network streams as fast, 6.42-6.44 vs 6.43-6.45 TB/s, and this form is a cross-check of
 *                 the signed network the fused pipelines use).  A zero
 *                 carries no sign through those: a result that is NEGATIVE zero in the reference's arithmetic (element 0 of a
 *                 row of negative zeros) comes back as +0; every other bit is unchanged
 *                 (tests/test_fwht_gpu.py::test_negative_zero_contract_of_both_launch_forms).  Other shapes ignore the bit.
 * Variants other than the ds_bpermute cross-check exist for f32 and D = 512..4096 only; elsewhere only
 * bit 0 (and bits 20..23) are honoured.  All variants produce identical bits, WHVI_FWHT_SIGNED_LANES up to the sign of zero
 * (tests/test_fwht_gpu.py).
 * The library reads NO environment variables: its launch form is a function of its arguments.
 */
#define WHVI_FWHT_SIGNED_LANES (1 << 23)
int whvi_fwht_ex(void *dst, const void *src, int64_t rows, int32_t log2d,
                 int32_t dtype, int32_t variant, void *stream);

/* Fused scale -> FWHT -> scale -> FWHT -> scale, one HBM read + one write per row:
 *
 *     dst[r, :] = A (.) FWHT( B_s (.) FWHT( C (.) src[r, :] ) ),   s = sample of row r
 *
 * replacing matmul_diag_left(s1, fwht(matmul_diag_left(u, fwht(X)))) of src/weights.py:73,84.
 * Every multiply is a separate IEEE rounding (no FMA contraction), as in the reference's
 * separate ATen kernels.  Row r belongs to MC sample s = (r / sample_stride) % n_samples.
 *
 *   axis = WHVI_AXIS_ROW : the reference-exact dataflow (matmul_diag_left scales ROWS,
 *       src/utils.py:4-12).  Rows form groups of group_rows (= D for a D x D weight
 *       matrix); with i = r % group_rows:  A = a[i], B_s = b[s*group_rows + i], C = c[i]
 *       (per-row scalars).
 *   axis = WHVI_AXIS_COL : the textbook S1.H.diag(g).H.S2 applied to row vectors
 *       (matmul_diag_right, src/utils.py:15-23): A = a[j], B_s = b[s*D + j], C = c[j]
 *       for column j (group_rows is ignored).
 *   a, b, c may each be NULL (treated as all ones, the multiply is skipped).
 *   src may be NULL only with axis = WHVI_AXIS_ROW and group_rows <= D: the input is then the
 *       first group_rows rows of the D x D identity per group, i.e. with c = s2 and
 *       group_rows = D it is torch.diag(s2) of src/weights.py:73 without materialising it (no
 *       HBM read at all); group_rows = 1 yields row 0 only (all WHVIColumnMatrix uses,
 *       src/weights.py:245).
 */
#define WHVI_AXIS_ROW 0
#define WHVI_AXIS_COL 1

int whvi_fused_shs_f32(void *dst, const void *src, const void *a, const void *b,
                       const void *c, int64_t rows, int32_t log2d, int64_t n_samples,
                       int64_t sample_stride, int64_t group_rows, int32_t axis,
                       void *stream);
int whvi_fused_shs_f64(void *dst, const void *src, const void *a, const void *b,
                       const void *c, int64_t rows, int32_t log2d, int64_t n_samples,
                       int64_t sample_stride, int64_t group_rows, int32_t axis,
                       void *stream);

/* Same pipeline with per-sample outer scale vectors, for batches of INDEPENDENT weight matrices
 * (the sub-matrices of WHVIStackedMatrix, src/weights.py:130-132,179-180, or several MC samples of
 * several layers in one launch): with the flag set, a (resp. c) is indexed like b,
 *     a[s*group_rows + i]  (axis = ROW)      a[s*D + j]  (axis = COL),
 * i.e. every "sample" s carries its own s1 / s2 / u.  flags == 0 is whvi_fused_shs_<dtype>. */
#define WHVI_FUSED_A_PER_SAMPLE 1
#define WHVI_FUSED_C_PER_SAMPLE 2
/* WHVI_FUSED_SRC_SHARED (axis = COL, D * sizeof >= 1 KiB, dst != src): src holds the rows of ONE sample -- sample_stride rows
 * -- shared by all samples; row r of dst is computed from src row r % sample_stride.  With rows in (sample, batch, D)
 * order (sample_stride = batch) this is a layer's first Monte-Carlo pass on a (batch, D) input: the input is read from
 * the caches instead of being expanded to (n_samples, batch, D) in HBM first.  Same arithmetic per row: same bits as the
 * launch on the expanded input. */
#define WHVI_FUSED_SRC_SHARED   4
/* WHVI_FUSED_ONE_TRANSFORM (axis = COL, D * sizeof >= 1 KiB, c == NULL): dst = A (.) FWHT(B_s (.) src) -- the second half of
 * the pipeline on its own (matmul_diag . fwht, src/utils.py:15-23 + src/fwht).  For a source shared by all samples the
 * first half FWHT(C (.) x) is sample-independent: compute it once (this entry with b = C, n_samples = 1), then every
 * sample with WHVI_FUSED_SRC_SHARED | WHVI_FUSED_ONE_TRANSFORM -- one transform per sample instead of two, the same
 * multiplies and butterflies in the same order, hence the same bits as the two-transform launch. */
#define WHVI_FUSED_ONE_TRANSFORM 8
/* WHVI_FUSED_RELU_IN / WHVI_FUSED_RELU_OUT (whvi_fused_shs_stacked_layer_f32, its 16-bit forms
 * whvi_fused_shs_stacked_layer_f16 / _bf16 and its backward, whvi_fused_shs_stacked_layer_bwd_f32 / _f16 / _bf16; every other
 * entry refuses them as unknown flags): an nn.ReLU in front of / behind the layer, applied on load / before the store -- max(., 0), NaN
 * passing; in the backward, the masks of those two. */
#define WHVI_FUSED_RELU_IN      16
#define WHVI_FUSED_RELU_OUT     32

int whvi_fused_shs_ex_f32(void *dst, const void *src, const void *a, const void *b,
                          const void *c, int64_t rows, int32_t log2d, int64_t n_samples,
                          int64_t sample_stride, int64_t group_rows, int32_t axis,
                          int32_t flags, void *stream);
int whvi_fused_shs_ex_f64(void *dst, const void *src, const void *a, const void *b,
                          const void *c, int64_t rows, int32_t log2d, int64_t n_samples,
                          int64_t sample_stride, int64_t group_rows, int32_t axis,
                          int32_t flags, void *stream);

/* The launch form whvi_fused_shs_ex_<dtype> (dtype: WHVI_F32, WHVI_F64, WHVI_F16 or WHVI_BF16) takes for these arguments on a
 * device of `cus` compute units (cus <= 0: the current device's count; cus > 0: no device is touched).  in_place: dst == src;
 * src_null / c_null: that pointer is NULL.  Returns WHVI_OK and writes, where the pointer is not NULL,
 *   *stage              which scale vectors a block stages in LDS: 0 none, 1 a and c, 3 a, b and c;
 *   *nt                 1 for the streaming (non-temporal) instantiation;
 *   *same_sample_blocks the kernel's block-map word: 0 consecutive tiles per block; 1 the four waves of a block take rows
 *                       n_samples apart (one sample per block, rows in (batch, sample, D) order); 2 a shared source's order,
 *                       the sample index fastest within an XCD;
 *   *grid               the blocks launched (0: nothing is launched).  A streaming launch whose grid is a multiple of 8 walks
 *                       its blocks in XCD-contiguous order unless same_sample_blocks is 2;
 * or returns the error code the launch returns for these arguments before it looks at a pointer's value (alignment and overlap
 * are the launch's to refuse).  Computed by the function the launch itself calls.  Launches nothing. */
int32_t whvi_fused_shs_plan(int32_t dtype, int64_t rows, int32_t log2d, int64_t n_samples, int64_t sample_stride,
                            int64_t group_rows, int32_t axis, int32_t flags, int32_t in_place, int32_t src_null, int32_t c_null,
                            int32_t cus, int32_t *stage, int32_t *nt, int32_t *same_sample_blocks, int64_t *grid);

/* Backward of whvi_fused_shs_f32 with axis = WHVI_AXIS_COL, shared a / c and per-sample b -- y = a (.) H(b_s (.) H(c (.) x)),
 * the fastfood layer -- in ONE launch plus a tiny finishing launch inside the same call.  float32.  Rows are in (sample, row, D)
 * order: n_samples * sample_stride rows, sample s holds rows [s * sample_stride, (s + 1) * sample_stride).  Per row:
 *     t1 = H(c x) (recomputed);  u = H(b_s t1), grad_a += grad_y u;  v = H(a grad_y), grad_b[s] += v t1;
 *     w = H(b_s v), grad_c += w x;  grad_x = c w
 *   grad_x : (n_samples * sample_stride, D), or NULL to skip the store.  Every multiply of its chain is its own rounding and the
 *            butterflies are the forward's: bit for bit whvi_fused_shs_f32(grad_x, grad_y, a := c, b, c := a, ...).
 *   grad_a, grad_c : (D), summed over all rows;  grad_b : (n_samples, D), summed over each sample's rows.  The sums are fused
 *            multiply-adds into registers; every block writes one partial per field to `work` and the finishing launch adds them
 *            in ascending block order: no atomics, bit-identical on every run.
 *   grad_y : (n_samples * sample_stride, D).  x : the same, or with flags = WHVI_FUSED_SRC_SHARED (sample_stride, D): row r of
 *            every sample reads x[r] (grad_x is still written per (sample, row): the caller sums over samples).
 *   a, c : (D);  b : (n_samples, D).
 *   work   : whvi_fused_shs_bwd_workspace(n_samples, sample_stride, log2d) bytes.  The query needs no device and depends on its
 *            arguments alone: 12 * D bytes per block of the launch, n_samples * n_slabs blocks, where the slabs per sample aim
 *            at 1024 blocks in all (512 at log2d = 12) and never go below four wave tiles (max(1, 1024 / D) rows each) per
 *            slab.  0 when n_samples * sample_stride == 0; WHVI_ERR_ARG for a negative size, WHVI_ERR_SIZE outside the range.
 * Supported: 6 <= log2d <= 12 -- whvi_fused_shs_bwd_supported(log2d) returns 1 exactly then (no device needed), the call
 * WHVI_ERR_SIZE otherwise.  flags other than 0 / WHVI_FUSED_SRC_SHARED: WHVI_ERR_ARG ("unknown fused flags").  Only grad_x may be
 * NULL (WHVI_ERR_ARG); every pointer 16-byte aligned (WHVI_ERR_ALIGN); grad_x, the parameter gradients and the workspace must
 * not overlap an input (WHVI_ERR_OVERLAP).  n_samples * sample_stride == 0 returns WHVI_OK without a launch or a write.  Every
 * argument check runs before any device call.  No allocation, no synchronisation: capture-safe.  whvi_last_kernel names
 * whvi::fused_shs_bwd_kernel<float, log2d, K, NT>. */
int     whvi_fused_shs_bwd_supported(int32_t log2d);
int64_t whvi_fused_shs_bwd_workspace(int64_t n_samples, int64_t sample_stride, int32_t log2d);
int     whvi_fused_shs_bwd_f32(void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *work,
                               const void *grad_y, const void *x, const void *a, const void *b, const void *c,
                               int64_t n_samples, int64_t sample_stride, int32_t log2d, int32_t flags, void *stream);

/* The same pipeline on 16-bit ACTIVATION streams: dst / src are IEEE half (_f16) or bfloat16 (_bf16), in place or out of
 * place; a, b, c are FLOAT32 vectors (they are the layer's float32 parameters; nothing is gained by rounding them).  Each
 * element is converted to f32 exactly, every multiply is its own f32 rounding, the butterflies are f32 adds / subs in the
 * reference's stage order, and the result is rounded to the storage type ONCE (round to nearest even; a bf16 NaN stays a
 * NaN), when the tile is stored: element for element the value of whvi_fused_shs_ex_f32 on the upcast input, cast once --
 * not the five roundings of the unfused 16-bit chain.  The sign of a zero result is exempt as it is for the f32 entry.
 * HBM traffic: 2 bytes read + 2 written per element.
 *   Supported: axis = WHVI_AXIS_COL with src != NULL, 3 <= log2d <= 13 (rows of one 16-byte chunk up to one wavefront tile),
 *   flags 0, WHVI_FUSED_A_PER_SAMPLE, WHVI_FUSED_C_PER_SAMPLE.  group_rows is checked (>= 1) and otherwise ignored.
 *   Refused with WHVI_ERR_ARG and a message naming the form: axis = WHVI_AXIS_ROW and src == NULL (the weight construction
 *   is float32), WHVI_FUSED_SRC_SHARED and WHVI_FUSED_ONE_TRANSFORM (a 16-bit intermediate between the two halves would be a
 *   second rounding).  log2d outside [3, 13]: WHVI_ERR_SIZE.  Otherwise the argument checks of whvi_fused_shs_ex_f32, and
 *   dst must not overlap a scale vector (WHVI_ERR_OVERLAP). */
int whvi_fused_shs_ex_f16 (void *dst, const void *src, const void *a, const void *b,
                           const void *c, int64_t rows, int32_t log2d, int64_t n_samples,
                           int64_t sample_stride, int64_t group_rows, int32_t axis,
                           int32_t flags, void *stream);
int whvi_fused_shs_ex_bf16(void *dst, const void *src, const void *a, const void *b,
                           const void *c, int64_t rows, int32_t log2d, int64_t n_samples,
                           int64_t sample_stride, int64_t group_rows, int32_t axis,
                           int32_t flags, void *stream);

/* whvi_fused_shs_bwd_f32 on 16-bit ACTIVATION streams: grad_x, grad_y and x are IEEE half (_f16) or bfloat16 (_bf16); a, b, c,
 * grad_a, grad_b, grad_c and the workspace stay FLOAT32.  The argument list, the flags (0 / WHVI_FUSED_SRC_SHARED), the layout
 * and every check are those of whvi_fused_shs_bwd_f32, with the extents of grad_x, grad_y and x counted in 2-byte elements.
 * whvi_fused_shs_bwd_supported and whvi_fused_shs_bwd_workspace serve the three entries unchanged: the grid and the slots do
 * not depend on the storage type.
 *   Rounding: every element of x and grad_y is converted to f32 exactly, the chain of whvi_fused_shs_bwd_f32 runs on those
 *   values -- every multiply its own f32 rounding, f32 butterflies in the forward's order, fused multiply-adds into f32 sums --
 *   and grad_x is rounded to the storage type ONCE (round to nearest even; a bf16 NaN stays a NaN) when it is stored.  Nothing
 *   is rounded to 16 bits in between.  Hence grad_x is element for element whvi_fused_shs_ex_f16 / _bf16(grad_x, grad_y,
 *   a := c, b, c := a, ...) (the sign of an exact zero is exempt, as for that entry), and the parameter gradients are the sums
 *   whvi_fused_shs_bwd_f32 forms on the upcast operands: bit for bit from log2d = 9 up, where every column adds the same rows
 *   in the same order; the same products in another lane order below.
 *   HBM traffic: 6 * D bytes per row -- x and grad_y read once, grad_x written once (4 * D with grad_x = NULL or a shared x
 *   that stays in cache) -- and no activation-sized temporary.
 * whvi_last_kernel names whvi::fused_shs_bwd_kernel<__half, log2d, K, NT> / <__hip_bfloat16, log2d, K, NT>. */
int     whvi_fused_shs_bwd_f16 (void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *work,
                                const void *grad_y, const void *x, const void *a, const void *b, const void *c,
                                int64_t n_samples, int64_t sample_stride, int32_t log2d, int32_t flags, void *stream);
int     whvi_fused_shs_bwd_bf16(void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *work,
                                const void *grad_y, const void *x, const void *a, const void *b, const void *c,
                                int64_t n_samples, int64_t sample_stride, int32_t log2d, int32_t flags, void *stream);

/* The rectangular fastfood layer: n_blocks (J) independent square operators applied to the SAME rows, their outputs written
 * side by side -- the paper's stacking of square blocks (src/weights.py: WHVIStackedMatrix.setup_dimensions) -- in ONE launch.
 * float32.  Rows are in (sample, row) order: n_samples * sample_stride rows, sample s holds rows [s * sample_stride,
 * (s + 1) * sample_stride).
 *     dst[r, j * D + n] = a[j, n] * H(b[j, s, :] (.) H(c[j, :] (.) src_row))[n]
 *   dst  : (n_samples * sample_stride, n_blocks * D).
 *   src  : (n_samples * sample_stride, D), or with flags = WHVI_FUSED_SRC_SHARED (sample_stride, D): row r reads
 *          src[r % sample_stride].
 *   a, c : (n_blocks, D);  b : (n_blocks, n_samples, D).
 * Every multiply is its own rounding and the transforms are the ones whvi_fused_shs_f32 runs: block j of dst is, element for
 * element, whvi_fused_shs_f32(src, a[j], b[j], c[j], axis = WHVI_AXIS_COL) -- non-finite inputs included, the sign of an exact
 * zero exempt as it is for that entry.  A row is read once and n_blocks segments are written: (1 + n_blocks) * D elements per
 * row, where n_blocks launches and a concatenation move about 4 * n_blocks * D.
 * Supported: 6 <= log2d <= 11, n_blocks >= 1 and 12 * D * n_blocks <= 65536 (every block of the launch stages all n_blocks
 * triples a_j, b_{j,s}, c_j in LDS) -- whvi_fused_shs_stacked_supported(log2d, n_blocks) returns 1 exactly then (no device
 * needed), the call WHVI_ERR_SIZE otherwise, as it does when n_samples * sample_stride >= 2^32.  flags other than 0 /
 * WHVI_FUSED_SRC_SHARED, a null pointer, a negative size: WHVI_ERR_ARG; a pointer that is not 16-byte aligned: WHVI_ERR_ALIGN;
 * dst overlapping any input: WHVI_ERR_OVERLAP.  n_samples * sample_stride == 0 returns WHVI_OK without a launch.  Every
 * argument check runs before any device call.  No atomics, no allocation, no synchronisation: capture-safe.  whvi_last_kernel
 * names whvi::fused_shs_stacked_kernel<float, log2d, K, NT>. */
int whvi_fused_shs_stacked_supported(int32_t log2d, int64_t n_blocks);
int whvi_fused_shs_stacked_f32(void *dst, const void *src, const void *a, const void *b, const void *c,
                               int64_t n_blocks, int64_t n_samples, int64_t sample_stride,
                               int32_t log2d, int32_t flags, void *stream);

/* whvi_fused_shs_stacked_f32 for 16-bit ACTIVATION storage: dst and src are float16 (_f16) or bfloat16 (_bf16), a, b, c stay
 * float32 -- the contract of whvi_fused_shs_ex_f16 / _bf16: the input is upcast exactly, every multiply is its own float32
 * rounding, the butterflies are float32, and each element is rounded to 16 bits ONCE, when it is stored.  Shapes, row order
 * and flags as above.  Block j of dst is, element for element, whvi_fused_shs_ex_f16 / _bf16(src, a[j], b[j], c[j], axis =
 * WHVI_AXIS_COL) -- with WHVI_FUSED_SRC_SHARED, that entry on the source repeated n_samples times (it has no shared-source
 * form) -- non-finite inputs included, the sign of an exact zero exempt.  A row is read once and n_blocks segments are written:
 * (1 + n_blocks) * D * 2 bytes per row.
 * Supported: whvi_fused_shs_stacked_f32's rule, 6 <= log2d <= 11, n_blocks >= 1 and 12 * D * n_blocks <= 65536 (the staged
 * vectors are float32) -- whvi_fused_shs_stacked16_supported(log2d, n_blocks) returns 1 exactly then (no device needed).  The
 * same checks in the same order and with the same codes as whvi_fused_shs_stacked_f32, the overlap check on byte extents of
 * 2-byte activations and 4-byte vectors, all before any device call; n_samples * sample_stride == 0 returns WHVI_OK without a
 * launch.  No atomics, no allocation, no synchronisation: capture-safe.  whvi_last_kernel names
 * whvi::fused_stacked16_kernel<__half | __hip_bfloat16, log2d, K, NT>. */
int whvi_fused_shs_stacked16_supported(int32_t log2d, int64_t n_blocks);
int whvi_fused_shs_stacked_f16(void *dst, const void *src, const void *a, const void *b, const void *c,
                               int64_t n_blocks, int64_t n_samples, int64_t sample_stride,
                               int32_t log2d, int32_t flags, void *stream);
int whvi_fused_shs_stacked_bf16(void *dst, const void *src, const void *a, const void *b, const void *c,
                                int64_t n_blocks, int64_t n_samples, int64_t sample_stride,
                                int32_t log2d, int32_t flags, void *stream);

/* whvi_fused_shs_stacked_f32 with what a network puts around the layer folded into the same launch: the activation in front,
 * the bias, the activation behind, and the narrowing to n_cols columns at a row pitch of the caller's.  float32.  Rows, src, a,
 * b, c as there.  For col = j * D + n < n_cols:
 *     dst[r * ld_dst + col] = act_out(a[j, n] * H(b[j, s, :] (.) H(c[j, :] (.) act_in(src_row)))[n] + bias[col])
 *   act_in / act_out : max(., 0) with NaN passing, as torch.relu (WHVI_FUSED_RELU_IN / WHVI_FUSED_RELU_OUT), else the identity.
 *   bias  : (n_blocks * D) floats, or NULL: the add is a rounding of its own behind the a multiply, and is skipped -- not
 *           "+ 0" -- without a bias.
 *   dst   : n_samples * sample_stride rows of pitch ld_dst floats.  Columns n_cols .. ld_dst - 1 of every row, and everything
 *           outside the rows, are not written.  n_cols and ld_dst are multiples of 4, (n_blocks - 1) * D < n_cols <=
 *           n_blocks * D (the narrowing ends in the last block) and ld_dst >= n_cols.
 * With bias == NULL, flags 0 / WHVI_FUSED_SRC_SHARED and n_cols == ld_dst == n_blocks * D the result is, bit for bit, that of
 * whvi_fused_shs_stacked_f32.  A row is read once and n_cols columns are written.
 * Supported: 6 <= log2d <= 11, n_blocks >= 1 and (12 + 4 * has_bias) * D * n_blocks <= 65536 (the bias is staged in LDS with the
 * triples) -- whvi_fused_shs_stacked_layer_supported(log2d, n_blocks, has_bias) returns 1 exactly then (no device needed), the
 * call WHVI_ERR_SIZE otherwise, as it does for an n_cols or ld_dst outside the rule above and when n_samples * sample_stride >=
 * 2^32.  Unknown flags, a negative size, a null pointer other than bias: WHVI_ERR_ARG; a pointer that is not 16-byte aligned:
 * WHVI_ERR_ALIGN; the rows * ld_dst floats of dst overlapping any input, the bias included: WHVI_ERR_OVERLAP.  n_samples *
 * sample_stride == 0 returns WHVI_OK without a launch.  Every argument check runs before any device call, in
 * whvi_fused_shs_stacked_f32's order.  No atomics, no allocation, no synchronisation: capture-safe.  whvi_last_kernel names
 * whvi::fused_shs_stacked_layer_kernel<float, log2d, K, NT>. */
int whvi_fused_shs_stacked_layer_supported(int32_t log2d, int64_t n_blocks, int32_t has_bias);
int whvi_fused_shs_stacked_layer_f32(void *dst, const void *src, const void *a, const void *b, const void *c,
                                     const void *bias /* (n_blocks * D) floats or NULL */,
                                     int64_t n_blocks, int64_t n_samples, int64_t sample_stride, int32_t log2d,
                                     int64_t n_cols, int64_t ld_dst, int32_t flags, void *stream);

/* whvi_fused_shs_stacked_layer_f32 for 16-bit ACTIVATION storage: dst and src are float16 (_f16) or bfloat16 (_bf16); a, b, c
 * and the bias stay float32 -- the contract of whvi_fused_shs_stacked_f16 / _bf16: the input is upcast exactly, act_in acts on
 * the upcast values, every multiply is its own float32 rounding, the butterflies are float32, the bias is added in float32 as a
 * rounding of its own (skipped without a bias), act_out acts on the float32 sum, and each element is rounded to 16 bits ONCE,
 * when it is stored: the result is whvi_fused_shs_stacked_layer_f32 on the upcast source, rounded once.  Shapes, row order,
 * flags (WHVI_FUSED_SRC_SHARED | WHVI_FUSED_RELU_IN | WHVI_FUSED_RELU_OUT) and the meaning of n_cols and ld_dst (in elements) as
 * there, except that n_cols and ld_dst are multiples of 8 -- a 16-byte chunk holds 8 columns.  With bias == NULL, flags 0 /
 * WHVI_FUSED_SRC_SHARED and n_cols == ld_dst == n_blocks * D the result is, bit for bit, that of whvi_fused_shs_stacked_f16 /
 * _bf16.  A row is read once and n_cols columns are written: (D + n_cols) * 2 bytes per row.
 * Supported: the float32 layer's rule, 6 <= log2d <= 11, n_blocks >= 1 and (12 + 4 * has_bias) * D * n_blocks <= 65536 --
 * whvi_fused_shs_stacked_layer16_supported(log2d, n_blocks, has_bias) returns 1 exactly then (no device needed).  The same
 * checks in the same order and with the same codes as whvi_fused_shs_stacked_layer_f32, the overlap check on byte extents of
 * 2-byte activations (rows * ld_dst of them for dst) and 4-byte vectors, every pointer 16-byte aligned, the bias included, all
 * before any device call; n_samples * sample_stride == 0 returns WHVI_OK without a launch.  No atomics, no allocation, no
 * synchronisation: capture-safe.  whvi_last_kernel names
 * whvi::fused_stacked16_layer_kernel<__half | __hip_bfloat16, log2d, K, NT>. */
int whvi_fused_shs_stacked_layer16_supported(int32_t log2d, int64_t n_blocks, int32_t has_bias);
int whvi_fused_shs_stacked_layer_f16(void *dst, const void *src, const void *a, const void *b, const void *c,
                                     const void *bias /* (n_blocks * D) floats or NULL */,
                                     int64_t n_blocks, int64_t n_samples, int64_t sample_stride, int32_t log2d,
                                     int64_t n_cols, int64_t ld_dst, int32_t flags, void *stream);
int whvi_fused_shs_stacked_layer_bf16(void *dst, const void *src, const void *a, const void *b, const void *c,
                                      const void *bias /* (n_blocks * D) floats or NULL */,
                                      int64_t n_blocks, int64_t n_samples, int64_t sample_stride, int32_t log2d,
                                      int64_t n_cols, int64_t ld_dst, int32_t flags, void *stream);

/* Backward of whvi_fused_shs_stacked_f32 in ONE launch plus a tiny finishing launch inside the same call.  float32.  Rows as
 * there.  Per row, for j = 0 .. n_blocks - 1, the chain of whvi_fused_shs_bwd_f32 on segment j of grad_y
 * (gy_j = grad_y[r, j * D : (j + 1) * D]):
 *     t1 = H(c_j x);  u = H(b_js t1), grad_a[j] += gy_j u;  v = H(a_j gy_j), grad_b[j, s] += v t1;
 *     w = H(b_js v), grad_c[j] += w x;  gx = c_0 w (j = 0), gx = gx + c_j w (j > 0: product and add are separate roundings)
 *   grad_x : (n_samples * sample_stride, D), stored once per row after the last j, or NULL to skip the store: bit for bit the
 *            grad_x of whvi_fused_shs_bwd_f32 per block, added in ascending j.
 *   grad_a, grad_c : (n_blocks, D);  grad_b : (n_blocks, n_samples, D).  Block j's three are, bit for bit, what
 *            whvi_fused_shs_bwd_f32 returns for a contiguous copy of segment j of grad_y with a[j], b[j], c[j]: the same
 *            operands, tiles, fused multiply-adds, per-block partials and finishing order (ascending block).  No atomics:
 *            bit-identical on every run.
 *   grad_y : (n_samples * sample_stride, n_blocks * D).  x : (n_samples * sample_stride, D), or with flags =
 *            WHVI_FUSED_SRC_SHARED (sample_stride, D): row r of every sample reads x[r] (grad_x is still written per
 *            (sample, row): the caller sums over samples).
 *   a, c : (n_blocks, D);  b : (n_blocks, n_samples, D).
 *   work   : whvi_fused_shs_stacked_bwd_workspace(n_samples, sample_stride, log2d, n_blocks) bytes = n_blocks times
 *            whvi_fused_shs_bwd_workspace(n_samples, sample_stride, log2d): one slot of 12 * D * n_blocks bytes per block of the
 *            launch, the grid being that call's.  The query needs no device and depends on its arguments alone.  0 when
 *            n_samples * sample_stride == 0; WHVI_ERR_ARG for a negative size, WHVI_ERR_SIZE outside the range.
 * A row of x and its n_blocks segments of grad_y are read once and grad_x is written once: (2 + n_blocks) * D elements per row.
 * Supported: 2 <= n_blocks <= 4 for 6 <= log2d <= 10, n_blocks = 2 at log2d = 11 -- whvi_fused_shs_stacked_bwd_supported(log2d,
 * n_blocks) returns 1 exactly then (no device needed), the call WHVI_ERR_SIZE otherwise (n_blocks = 1 is
 * whvi_fused_shs_bwd_f32), as it does when n_samples * sample_stride >= 2^32 or n_blocks * (n_samples + 2) * D >= 2^31.  flags
 * other than 0 / WHVI_FUSED_SRC_SHARED, a negative size, a null pointer other than grad_x: WHVI_ERR_ARG; a pointer that is not
 * 16-byte aligned: WHVI_ERR_ALIGN; grad_x, a parameter gradient or the workspace overlapping an input: WHVI_ERR_OVERLAP.
 * n_samples * sample_stride == 0 returns WHVI_OK without a launch or a write.  Every argument check runs before any device
 * call.  No allocation, no synchronisation: capture-safe.  whvi_last_kernel names
 * whvi::fused_shs_stacked_bwd_kernel<float, log2d, K, n_blocks, NT>. */
int     whvi_fused_shs_stacked_bwd_supported(int32_t log2d, int64_t n_blocks);
int64_t whvi_fused_shs_stacked_bwd_workspace(int64_t n_samples, int64_t sample_stride, int32_t log2d, int64_t n_blocks);
int     whvi_fused_shs_stacked_bwd_f32(void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *work,
                                       const void *grad_y, const void *x, const void *a, const void *b, const void *c,
                                       int64_t n_blocks, int64_t n_samples, int64_t sample_stride,
                                       int32_t log2d, int32_t flags, void *stream);

/* Backward of whvi_fused_shs_stacked_f16 / _bf16 in ONE launch plus a tiny finishing launch inside the same call: the call above
 * on 16-bit activation streams.  grad_y, x and grad_x are __half / __hip_bfloat16; a, b, c, grad_a, grad_b, grad_c and work are
 * float32.  The chain above runs in float32 on the exactly-upcast x and grad_y; gx stays float32 across the n_blocks segments
 * and grad_x is rounded to 16 bits ONCE, when it is stored after the last j: whvi_fused_shs_stacked_bwd_f32 on the upcasts,
 * cast once (the per-block launches of whvi_fused_shs_bwd_f16 / _bf16 added in 16 bits round 2 * n_blocks - 1 times).  Block
 * j's grad_a, grad_b, grad_c are, bit for bit, what whvi_fused_shs_bwd_f16 / _bf16 returns for a contiguous copy of segment j of
 * grad_y with a[j], b[j], c[j], and from log2d = 9 up the float32 call's on the upcasts.  No atomics: bit-identical on every
 * run.  Shapes, flags and the workspace (whvi_fused_shs_stacked_bwd_workspace, unchanged: the grid and the slots are the
 * same) as above; (2 + n_blocks) * D * 2 bytes per row.
 * Supported: the float32 call's rule, 2 <= n_blocks <= 4 for 6 <= log2d <= 10, n_blocks = 2 at log2d = 11 --
 * whvi_fused_shs_stacked_bwd16_supported(log2d, n_blocks) returns 1 exactly then (no device needed).  The same checks in the
 * same order and with the same codes as whvi_fused_shs_stacked_bwd_f32, the overlap check on byte extents of 2-byte
 * activations and 4-byte vectors, all before any device call; n_samples * sample_stride == 0 returns WHVI_OK without a launch
 * or a write.  No allocation, no synchronisation: capture-safe.  whvi_last_kernel names
 * whvi::fused_stacked_bwd16_kernel<__half | __hip_bfloat16, log2d, K, n_blocks, NT>. */
int whvi_fused_shs_stacked_bwd16_supported(int32_t log2d, int64_t n_blocks);
int whvi_fused_shs_stacked_bwd_f16(void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *work,
                                   const void *grad_y, const void *x, const void *a, const void *b, const void *c,
                                   int64_t n_blocks, int64_t n_samples, int64_t sample_stride,
                                   int32_t log2d, int32_t flags, void *stream);
int whvi_fused_shs_stacked_bwd_bf16(void *grad_x, void *grad_a, void *grad_b, void *grad_c, void *work,
                                    const void *grad_y, const void *x, const void *a, const void *b, const void *c,
                                    int64_t n_blocks, int64_t n_samples, int64_t sample_stride,
                                    int32_t log2d, int32_t flags, void *stream);

/* Backward of whvi_fused_shs_stacked_layer_f32 in ONE launch plus a tiny finishing launch inside the same call: the call above
 * with the layer's epilogue folded in -- the masks of both ReLUs, the zero padding past n_cols and the bias sum.  float32.
 * Per row, for j = 0 .. n_blocks - 1 and col = j * D + n:
 *     xin    = WHVI_FUSED_RELU_IN ? max(x, 0) (NaN passing) : x
 *     g_j[n] = 0 for col >= n_cols (those 16-byte chunks of grad_y and y are not read), elsewhere
 *              WHVI_FUSED_RELU_OUT ? (y[col] <= 0 ? +0 : grad_y[col]) : grad_y[col]   -- a select, aten.threshold_backward:
 *              a NaN y passes grad_y, y = -0 gives 0, a NaN grad_y under y <= 0 gives 0
 *     grad_bias[col] += g_j[n];  the chain of whvi_fused_shs_stacked_bwd_f32 on (xin, g_j), the zero chunks included
 *     grad_x = WHVI_FUSED_RELU_IN ? (xin <= 0 ? +0 : gx) : gx, stored once per row, or not at all with grad_x == NULL
 *   grad_y, y : (n_samples * sample_stride, n_cols) at a common row pitch of ld floats; columns n_cols .. ld - 1 are never
 *            read.  y (the forward's output) is given exactly with WHVI_FUSED_RELU_OUT and NULL otherwise.
 *   x, a, b, c, grad_a, grad_b, grad_c : as in whvi_fused_shs_stacked_bwd_f32.
 *   grad_bias : (n_blocks * D) floats or NULL (no sum at all); all n_blocks * D entries are written, those from n_cols on as +0.
 *   work   : whvi_fused_shs_stacked_layer_bwd_workspace(n_samples, sample_stride, log2d, n_blocks, has_bias) bytes: one slot of
 *            (12 + 4 * has_bias) * D * n_blocks bytes per block of the launch (the grid of whvi_fused_shs_bwd_f32).  0 when
 *            n_samples * sample_stride == 0; WHVI_ERR_ARG for a negative size, WHVI_ERR_SIZE outside the range.
 * grad_x, grad_a, grad_b, grad_c are, bit for bit, whvi_fused_shs_stacked_bwd_f32 on the masked, zero-padded g and on
 * relu(x), followed by the mask on grad_x.  grad_bias is each lane's plain float sum in tile order, then the reductions of
 * grad_a (same-column butterfly, wave order, ascending block): deterministic, its own summation order.  No atomics.
 * Supported: 2 <= n_blocks <= 4 for 6 <= log2d <= 10, n_blocks = 2 at log2d = 11, with or without a bias --
 * whvi_fused_shs_stacked_layer_bwd_supported(log2d, n_blocks, has_bias) returns 1 exactly then (no device needed).  Checks, all
 * before any device call: flags outside WHVI_FUSED_SRC_SHARED | WHVI_FUSED_RELU_IN | WHVI_FUSED_RELU_OUT or a negative size
 * WHVI_ERR_ARG; an unsupported (log2d, n_blocks, has_bias), n_cols or ld not a multiple of 4, n_cols outside
 * ((n_blocks - 1) * D, n_blocks * D], ld < n_cols or ld >= 2^32 WHVI_ERR_SIZE; n_samples * sample_stride == 0 WHVI_OK without a launch or a
 * write; a null pointer other than grad_x / grad_bias, a null y with WHVI_FUSED_RELU_OUT, a y without it WHVI_ERR_ARG;
 * n_samples * sample_stride >= 2^32, rows * ld > 2^60 or n_blocks * (n_samples + 2 + has_bias) * D >= 2^31 WHVI_ERR_SIZE; a misaligned pointer
 * WHVI_ERR_ALIGN; an output or the workspace overlapping an input (rows * ld floats for grad_y and y) WHVI_ERR_OVERLAP.  No
 * allocation, no synchronisation: capture-safe.  whvi_last_kernel names
 * whvi::fused_shs_stacked_layer_bwd_kernel<float, log2d, K, n_blocks, has_bias, NT>. */
int     whvi_fused_shs_stacked_layer_bwd_supported(int32_t log2d, int64_t n_blocks, int32_t has_bias);
int64_t whvi_fused_shs_stacked_layer_bwd_workspace(int64_t n_samples, int64_t sample_stride, int32_t log2d,
                                                   int64_t n_blocks, int32_t has_bias);
int     whvi_fused_shs_stacked_layer_bwd_f32(void *grad_x /* or NULL */, void *grad_a, void *grad_b, void *grad_c,
                                             void *grad_bias /* (n_blocks * D) floats or NULL */, void *work,
                                             const void *grad_y, const void *y /* NULL unless WHVI_FUSED_RELU_OUT */,
                                             const void *x, const void *a, const void *b, const void *c,
                                             int64_t n_blocks, int64_t n_samples, int64_t sample_stride, int32_t log2d,
                                             int64_t n_cols, int64_t ld, int32_t flags, void *stream);

/* Backward of whvi_fused_shs_stacked_layer_f16 / _bf16 in ONE launch plus a tiny finishing launch inside the same call: the call
 * above on 16-bit activation streams -- its contract on the arithmetic of whvi_fused_shs_stacked_bwd_f16 / _bf16.  grad_y, y, x
 * and grad_x are __half / __hip_bfloat16; a, b, c, grad_a, grad_b, grad_c, grad_bias and work are float32.  x, grad_y and y are
 * upcast exactly on load; xin, the select g_j (aten.threshold_backward's semantics, as above), the bias sum and the chain are
 * float32, nothing is rounded to 16 bits in between; gx stays float32 across the n_blocks segments and
 *     grad_x = WHVI_FUSED_RELU_IN ? (xin <= 0 ? +0 : round16(gx)) : round16(gx)
 * is rounded ONCE and stored once per row, or not at all with grad_x == NULL.
 *   grad_y, y : (n_samples * sample_stride, n_cols) at a common row pitch of ld 2-byte elements; n_cols and ld are multiples of
 *            8 (a 16-byte chunk); columns n_cols .. ld - 1 and the chunks of the last block past n_cols are never read.
 *   grad_bias : (n_blocks * D) floats or NULL; all n_blocks * D entries are written, those from n_cols on as +0.
 *   work   : whvi_fused_shs_stacked_layer_bwd_workspace(...) bytes, unchanged: the grid and the slot of (12 + 4 * has_bias) * D *
 *            n_blocks bytes are the float32 call's.
 * grad_x, grad_a, grad_b, grad_c are, bit for bit, whvi_fused_shs_stacked_bwd_f16 / _bf16 on the masked, zero-padded 16-bit g
 * and on relu(x), followed by the 16-bit mask on grad_x (the select commutes with the one rounding, and the masked 16-bit values
 * are exact); with no flag, grad_bias == NULL and n_cols == ld == n_blocks * D the call has that entry's bits.  grad_bias is the
 * float32 sum of the masked gradient in the order described above: deterministic, its own summation order.  No atomics.
 * (2 * D + (1 + [ReLU out]) * n_cols) * 2 bytes per row.
 * Supported: 2 <= n_blocks <= 4 for 6 <= log2d <= 10, n_blocks = 2 at log2d = 11, with or without a bias --
 * whvi_fused_shs_stacked_layer_bwd16_supported(log2d, n_blocks, has_bias) returns 1 exactly then (no device needed).  The checks
 * of whvi_fused_shs_stacked_layer_bwd_f32 in its order and with its codes, all before any device call, with n_cols and ld
 * multiples of 8, the extents of grad_y, y (rows * ld), x and grad_x counted in 2-byte elements and those of the vectors in
 * 4-byte elements; n_samples * sample_stride == 0 returns WHVI_OK without a launch or a write.  No allocation, no
 * synchronisation: capture-safe.  whvi_last_kernel names
 * whvi::fused_layer_bwd16_kernel<__half | __hip_bfloat16, log2d, K, n_blocks, has_bias, NT>. */
int whvi_fused_shs_stacked_layer_bwd16_supported(int32_t log2d, int64_t n_blocks, int32_t has_bias);
int whvi_fused_shs_stacked_layer_bwd_f16(void *grad_x /* or NULL */, void *grad_a, void *grad_b, void *grad_c,
                                         void *grad_bias /* (n_blocks * D) floats or NULL */, void *work,
                                         const void *grad_y, const void *y /* NULL unless WHVI_FUSED_RELU_OUT */,
                                         const void *x, const void *a, const void *b, const void *c,
                                         int64_t n_blocks, int64_t n_samples, int64_t sample_stride, int32_t log2d,
                                         int64_t n_cols, int64_t ld, int32_t flags, void *stream);
int whvi_fused_shs_stacked_layer_bwd_bf16(void *grad_x /* or NULL */, void *grad_a, void *grad_b, void *grad_c,
                                          void *grad_bias /* (n_blocks * D) floats or NULL */, void *work,
                                          const void *grad_y, const void *y /* NULL unless WHVI_FUSED_RELU_OUT */,
                                          const void *x, const void *a, const void *b, const void *c,
                                          int64_t n_blocks, int64_t n_samples, int64_t sample_stride, int32_t log2d,
                                          int64_t n_cols, int64_t ld, int32_t flags, void *stream);

/* Reparameterisation + KL of J weight matrices in ONE launch, replacing the reference's
 * chain of small ATen kernels: g_sigma = softplus(g_rho) (src/weights.py:43-50), g_sigma * eps per MC sample
 * (src/weights.py:82-83,92), and kl_diag_normal(g_mu, g_sigma, 0, lambda) (src/weights.py:52-64,
 * src/utils.py:49-71, reference argument convention kept).  All buffers f32, contiguous:
 *   g_mu, g_rho : (J, D)        eps : (J, S, D)  drawn by the caller (injectable, graph-safe)
 *   u           : (J, 1+S, D)   u[j,0] = g_mu[j],  u[j,1+k] = sigma[j] * eps[j,k]   -> b of whvi_fused_shs_ex
 *   sigma       : (J, D)        kept for the backward pass
 *   kl_part     : (J, whvi_reparam_kl_blocks(D))  per-block partial sums; KL[j] = sum over the last axis
 */
int whvi_reparam_kl_blocks(int64_t D);
int whvi_reparam_kl_f32(void *u, void *sigma, void *kl_part, const void *g_mu, const void *g_rho,
                        const void *eps, int64_t J, int64_t S, int64_t D, float lambda_, void *stream);

/* The weight construction itself as a dedicated launch (src/weights.py:73; the generic route is
 * whvi_fused_shs_ex with src == NULL -- same bits):
 *     dst[j,k,i,:] = s1[j,i] * fwht( u[j,k,i] * fwht(s2[j,i] e_i) )  (+ base[j,i,:])
 * for the first R <= D rows i of each of the J x S matrices.  fwht(s2_i e_i) = s2_i H[i,:] is generated from bit
 * parities (the butterflies of a one-hot row are exact), so each row costs ONE transform, no HBM read, one write.
 * `base` (J, R, D), optional: a matrix added to every sample's matrix in the epilogue -- with base =
 * w_bar(g_mu) from a first call this is `w_bar(g_mu) + w_bar(g_sigma * eps_k)` of src/weights.py:93 without a
 * separate read-modify-write pass over all weight matrices.
 *   s1, s2 : (J, D)     dst : (J, S, R, D)     log2d in [2, 13] (f32) / [1, 12] (f64)
 *   u : (J, u_group, D); matrix (j, k) uses row u_first + k of group j.  u_group = S, u_first = 0 is the plain
 *       (J, S, D) layout; with the (J, 1 + S, D) buffer of whvi_reparam_kl the mean call passes S = 1, u_first = 0 and
 *       the per-sample call u_first = 1, both with u_group = 1 + S_samples -- no slicing copies. */
int whvi_wbar_fwd_f32(void *dst, const void *s1, const void *u, const void *s2, const void *base,
                      int64_t J, int64_t S, int64_t R, int32_t log2d, int64_t u_group, int64_t u_first,
                      void *stream);
int whvi_wbar_fwd_f64(void *dst, const void *s1, const void *u, const void *s2, const void *base,
                      int64_t J, int64_t S, int64_t R, int32_t log2d, int64_t u_group, int64_t u_first,
                      void *stream);

/* `w_bar(g_mu) + w_bar(g_sigma * eps_k)` of src/weights.py:93 in ONE launch: u is (J, 1 + S, D) -- row 0 of each group the
 * mean vector, rows 1 .. S the samples (the buffer whvi_reparam_kl writes) -- and
 *     dst[j,k,i,:] = s1[j,i] * fwht(u[j,0,i] * fwht(s2[j,i] e_i))  +  s1[j,i] * fwht(u[j,1+k,i] * fwht(s2[j,i] e_i)),
 * both terms computed by the same wave (two in-register transforms per tile, no mean matrix in memory).  The same
 * multiplies, butterflies and final add as whvi_wbar_fwd twice (mean matrix, then samples with `base`): the same bits.
 * Meant for cache-resident results (a launch and the re-read of the mean matrix saved); streams keep the two-launch
 * form, which does half the arithmetic per byte written.   dst : (J, S, R, D); log2d in [2, 12] (f32) / [1, 11] (f64):
 * two 64-register tiles per wave -- longer rows return WHVI_ERR_SIZE (use whvi_wbar_fwd with `base`). */
int whvi_wbar_fwd_mean_f32(void *dst, const void *s1, const void *u, const void *s2, int64_t J, int64_t S, int64_t R,
                           int32_t log2d, void *stream);
int whvi_wbar_fwd_mean_f64(void *dst, const void *s1, const void *u, const void *s2, int64_t J, int64_t S, int64_t R,
                           int32_t log2d, void *stream);

/* Backward of the weight construction in ONE launch: reads the incoming gradient once, writes three scalars per
 * row.  The reference obtains the same quantities from autograd over its op chain (matmul_diag_left backward,
 * src/utils.py:4-12, and FWHTFunction.backward = FWHT, src/fwht/cuda/fwht.py:14-16): four more FWHT launches and
 * ~10 elementwise / reduction launches over (J, S, R, D) tensors.  Buffers of the entry point's dtype, contiguous:
 *   grad_w  : (J, S, R, D)  dL/dW, first R <= D rows of every matrix      s1, s2 : (J, D)      u : (J, S, D)
 *   grad_u  : (J, S, D)     dL/du[j,k,i] for i < R; entries i >= R are NOT written (zero-fill them when R < D)
 *   part_s1 : (J, S, D)     per-sample contributions, same convention; dL/ds1[j,i] = sum over k (likewise part_s2)
 * flags = WHVI_WBAR_MEAN: W[j,k] = w_bar(u[j,0]) + w_bar(u[j,1+k]) (the whvi_wbar_fwd `base` form): u and the three
 *   outputs are (J, 1 + S, D); rows 1..S are written (part_s1 / part_s2 include the mean vector's share) and row 0 is
 *   left to the caller: the sum over k of rows 1..S is dL/du[j,0] resp. the per-matrix totals.
 * log2d in [2, 13] (f32) / [1, 12] (f64). */
#define WHVI_WBAR_MEAN   1
#define WHVI_WBAR_NO_LDS 2   /* tuning / cross-check: butterflies through the DPP network instead of the LDS-staged one
                              * (same adds in the same order: identical transform bits) */
#define WHVI_WBAR_SMALL_TILES 4   /* tuning / cross-check: force the quarter-size tiles small problems take ... */
#define WHVI_WBAR_BIG_TILES   8   /* ... or forbid them (default: chosen by size) */
int whvi_wbar_bwd_f32(void *grad_u, void *part_s1, void *part_s2, const void *grad_w, const void *s1,
                      const void *u, const void *s2, int64_t J, int64_t S, int64_t R, int32_t log2d,
                      int32_t flags, void *stream);
int whvi_wbar_bwd_f64(void *grad_u, void *part_s1, void *part_s2, const void *grad_w, const void *s1,
                      const void *u, const void *s2, int64_t J, int64_t S, int64_t R, int32_t log2d,
                      int32_t flags, void *stream);

/* `h @ (w_bar(g_mu) + w_bar(g_sigma * eps_k)).T (+ bias)` of src/weights.py:87-93,101-102 for all MC samples in ONE launch,
 * without building the matrices.  As written in the reference w_bar(u) = S1 . fwht(diag(u) . fwht(diag(s2))) is EXACTLY
 * D * diag(s1 (.) u (.) s2) -- row scales around row transforms, SURVEY.md finding 1 -- so the dense product adds exact zeros
 * to one product per output.  This entry computes that product directly, with the roundings of the as-written chain in the
 * same order ( v = u_i * s2_i;  D * v exact;  s1_i * .;  mean + sample;  h * w;  + bias ):
 *     out[k, b, i] = x[(k,) b, i] * ( wd(u[0])_i + wd(u[1 + k])_i ) + bias[i],     wd(u)_i = s1_i * (D * (u_i * s2_i)),
 * identical to the matrix route (weight construction + GEMM) for every input -- bit for bit against rocBLAS on MI355X, zeros
 * included: the product is added to +0, the value the other D - 1 products (exact zeros) sum to in a GEMM's +0-initialised
 * accumulator, so a product of -0 comes out as +0 like there.  Non-finite operands are propagated as the matrix
 * route propagates them: a row of x holding an inf / NaN at column j makes every other output of that row NaN (inf * 0 in
 * the dot product), a non-finite s1_i or an overflowing partial sum of the second transform (|D/2 * u_i * s2_i| = inf) makes
 * output column i NaN.
 *   x    : (S, B, D), or (B, D) with WHVI_DIAG_X_SHARED (a layer's first pass: one input for all samples; dst must not overlap)
 *   u    : (1 + S, D) with WHVI_DIAG_MEAN_PLUS (row 0 = g_mu, row 1 + k = g_sigma * eps_k: the buffer whvi_reparam_kl
 *          writes), else (S, D) and w_k = wd(u[k]) alone (direct weight sampling, src/weights.py:75-85,104-108)
 *   s1, s2 : (D,)    bias : (D,) or NULL    out : (S, B, D); out == x is allowed without WHVI_DIAG_X_SHARED
 *   log2d in [2, 12] (f32) / [1, 11] (f64). */
#define WHVI_DIAG_X_SHARED  1
#define WHVI_DIAG_MEAN_PLUS 2
/* Element-wise neighbours fused in (an nn.ReLU in front of / behind the layer in the caller's nn.Sequential, src/networks.py:49
 * running the reference's module list): x is passed through max(x, 0) on load, resp. the result before the store -- the
 * values torch.relu gives (NaN stays NaN), one read + one write of the activations instead of three. */
#define WHVI_DIAG_RELU_IN   4
#define WHVI_DIAG_RELU_OUT  8
/* tuning / cross-check (same values either way): force the streaming (non-temporal) or the cached launch instead of the
 * choice by size; keep the plain block order on a shared input */
#define WHVI_DIAG_TUNE_NT          16
#define WHVI_DIAG_TUNE_CACHED      32
#define WHVI_DIAG_TUNE_PLAIN_ORDER 64
#define WHVI_DIAG_TUNE_BIG_TILES   128   /* 16 KiB tiles at cache-resident sizes too (default there: quarter-size tiles) */
#define WHVI_DIAG_TUNE_MASK        (16 | 32 | 64 | 128)
int whvi_diag_apply_f32(void *out, const void *x, const void *s1, const void *s2, const void *u, const void *bias,
                        int64_t S, int64_t B, int32_t log2d, int32_t flags, void *stream);
int whvi_diag_apply_f64(void *out, const void *x, const void *s1, const void *s2, const void *u, const void *bias,
                        int64_t S, int64_t B, int32_t log2d, int32_t flags, void *stream);
/* The order in which the launch of whvi_diag_apply_<dtype>(S, B, log2d, flags) -- with out == x when in_place is non-zero --
 * walks its tiles.  The values are the same in every order; the order decides which XCD's L2 sees which tile, and a test
 * needs it to know which block map of the kernel a launch exercised (whvi_last_kernel names the instantiation only: the
 * order also depends on the grid).  Computed by the function the launch itself uses; launches nothing, needs no device.
 *   WHVI_DIAG_ORDER_PLAIN          block b takes tile group b
 *   WHVI_DIAG_ORDER_XCD            streaming launch, grid a multiple of 8: the blocks of one XCD walk a contiguous eighth
 *   WHVI_DIAG_ORDER_SAMPLE_FASTEST streaming launch on a shared input with S > 1, every sample a whole number of 8-block
 *                                  groups, no WHVI_DIAG_TUNE_PLAIN_ORDER: an XCD runs each of its row groups for all samples
 *                                  back to back (the input tile is fetched into that XCD's L2 once)
 * Negative: the error code whvi_diag_apply returns for these arguments before it launches (unknown dtype or flags, log2d
 * out of range, 2^32 rows or more, a shared input in place).  S * B == 0 (nothing is launched) reports the plain order. */
#define WHVI_DIAG_ORDER_PLAIN          0
#define WHVI_DIAG_ORDER_XCD            1
#define WHVI_DIAG_ORDER_SAMPLE_FASTEST 2
int32_t whvi_diag_apply_order(int32_t dtype, int64_t S, int64_t B, int32_t log2d, int32_t flags, int32_t in_place);

/* Backward of whvi_diag_apply (closed form; replaces autograd over the GEMM, the weight construction and its op chain):
 *   grad_x : (S, B, D) = g[k, b, :] (.) w_k, or NULL when the input needs no gradient (with WHVI_DIAG_X_SHARED the caller
 *            sums it over k)
 *   out    : (4, U, D), U = S (+ 1 with WHVI_DIAG_MEAN_PLUS); row r = k (+ 1) of slot 0 = dL/du[r], of slots 1 / 2 = sample
 *            k's share of dL/ds1 / dL/ds2, of slot 3 = its share of dL/dbias = sum_b g[k, b, :].  With the mean row, row 0
 *            is left to the caller: the sum of rows 1 .. S is dL/du[0] resp. the totals (one reduction for all four).
 *   part   : workspace of S * n_slabs * 2 * D elements, n_slabs = whvi_diag_apply_bwd_slabs(dtype, S, B, log2d) -- the
 *            batch reduction sum_b g (.) x runs over n_slabs row slabs per sample, combined in slab order by a second,
 *            tiny launch inside the same call (deterministic summation order; no atomics).
 * Non-finite g propagates element-wise (no attempt to mimic the matrix route on a diverged backward pass).
 * x is the forward's input as it was passed (BEFORE a fused WHVI_DIAG_RELU_IN); bias (the forward's, or NULL) is read only with
 * WHVI_DIAG_RELU_OUT, whose mask is recomputed from x, the diagonal and the bias with the forward's roundings (torch's
 * threshold_backward: the gradient passes unless the activation's result is <= 0). */
int64_t whvi_diag_apply_bwd_slabs(int32_t dtype, int64_t S, int64_t B, int32_t log2d);
int whvi_diag_apply_bwd_f32(void *grad_x, void *out, void *part, const void *g, const void *x, const void *s1,
                            const void *s2, const void *u, const void *bias, int64_t S, int64_t B, int32_t log2d,
                            int64_t n_slabs, int32_t flags, void *stream);
int whvi_diag_apply_bwd_f64(void *grad_x, void *out, void *part, const void *g, const void *x, const void *s1,
                            const void *s2, const void *u, const void *bias, int64_t S, int64_t B, int32_t log2d,
                            int64_t n_slabs, int32_t flags, void *stream);

/* The batched pass of a reference-mode stacked layer (WHVIStackedMatrix, src/weights.py:111-208) of any width without its
 * matrices: the stacked weight is J square blocks, each exactly diagonal as written, and ONE launch writes all of them (f32):
 *     out[s, b, j D + i] = relu?( relu?(x[(s,) b, i]) * w[j, s, i] + 0 (+ bias[j D + i]) )     j < J, i < D, j D + i < n_cols
 *     w[j, s, i] = wd_j(u[j, 0])_i + wd_j(u[j, 1 + s])_i,     wd_j(v)_i = s1[j, i] * (D * (v_i * s2[j, i]))
 * with whvi_diag_apply_f32's arithmetic and non-finite rules per block (bit-identical to that launch per block, concatenated and
 * narrowed to n_cols): a row of x with a non-finite entry at column k, tested after WHVI_DIAG_RELU_IN, has its outputs i != k
 * NaN in EVERY block and output k of each block the plain product; two such entries make the whole row NaN.
 *   x      : (S B, D) in (sample, row) order, or (B, D) with WHVI_DIAG_X_SHARED        s1, s2 : (J, D)
 *   u      : (J, 1 + S, D) with WHVI_DIAG_MEAN_PLUS (whvi_reparam_kl's buffer), else (J, S, D) and w = wd_j(u[j, s]) alone
 *   bias   : J D floats or NULL
 *   out    : S B rows at pitch ld_out >= n_cols floats; exactly n_cols columns of each row are written, 1 <= n_cols <= J D,
 *            columns n_cols .. ld_out - 1 are not touched.  16-byte stores where out is 16-byte aligned and ld_out a multiple
 *            of 4 (dword stores for a ragged last chunk or another pitch); non-temporal above 256 MiB written.
 *   flags  : WHVI_DIAG_X_SHARED, _MEAN_PLUS, _RELU_IN, _RELU_OUT; WHVI_DIAG_TUNE_NT / _CACHED force the store form (cross-checks)
 * Supported (whvi_diag_apply_stacked_supported): log2d in [2, 12], n_blocks >= 1 and one sample's diagonals and bias within
 * 64 KiB of LDS, 8 J D <= 65536; anything else returns WHVI_ERR_SIZE.  Inputs 16-byte aligned, out 4-byte; out must not
 * overlap an input (no in-place use); S B < 2^32.  S B == 0 returns WHVI_OK without a launch. */
int whvi_diag_apply_stacked_supported(int32_t log2d, int64_t n_blocks);
int whvi_diag_apply_stacked_f32(void *out, const void *x, const void *s1, const void *s2, const void *u, const void *bias,
                                int64_t S, int64_t B, int32_t log2d, int64_t n_blocks, int64_t n_cols, int64_t ld_out,
                                int32_t flags, void *stream);

/* Backward of whvi_diag_apply_stacked_f32 in one call (f32; closed form on the n_cols columns that were written).  With
 * w[j, s, :] the forward's diagonal (same roundings) and gm = g masked by the output activation:
 *   grad_x : (S, B, D), grad_x[s, b, i] = [WHVI_DIAG_RELU_IN: x > 0] * sum_{j : j D + i < n_cols} gm[s, b, j D + i] * w[j, s, i]
 *            -- separate float32 multiplies and adds, in ascending j; +0 where no written column reaches; NULL when the input
 *            needs no gradient.  With WHVI_DIAG_X_SHARED it is still (S, B, D) and the caller sums it over s.  Non-temporal
 *            stores above 256 MiB written (WHVI_DIAG_TUNE_NT / _CACHED force the store form).
 *   out    : (4, J, U, D), U = S (+ 1 with WHVI_DIAG_MEAN_PLUS): whvi_diag_apply_bwd's (4, U, D) layout per block -- slot 0
 *            dL/du[j, r], slots 1 / 2 sample k's share of dL/ds1[j] / dL/ds2[j] (that call's expressions), slot 3 its share
 *            of dL/dbias[j D + i] = sum_b gm; with the mean row, row 0 is left to the caller (the sum of rows 1 .. S).  Columns
 *            j D + i >= n_cols hold zeros in all four slots.
 *   part   : workspace of S * n_slabs * 2 * C floats, C = 4 * ceil(n_cols / 4) (the written columns: 8 floats per slab for an
 *            n -> 2 layer, 2 J D at most), n_slabs = whvi_diag_apply_stacked_bwd_slabs(S, B, log2d, J, n_cols): the batch sums
 *            run over n_slabs row slabs per sample, combined in slab order by a small finishing launch inside the same call
 *            (deterministic order, no atomics).
 *   g      : S B rows at pitch ld_g >= n_cols floats, n_cols columns of each read (4-byte aligned; 16-byte loads where g is
 *            16-byte aligned and ld_g a multiple of 4, dword loads otherwise and for a ragged last chunk)
 *   x      : the forward's input as it was passed (before a fused WHVI_DIAG_RELU_IN); columns that no written column
 *            multiplies are not read.          bias : the forward's (J D floats) or NULL, read only with WHVI_DIAG_RELU_OUT
 * The output activation's mask is recomputed from x, the diagonal and the bias with the forward's roundings, z = relu?(x) * w
 * + 0 (+ bias): the gradient passes unless relu(z) <= 0 -- on finite data the mask `out > 0` of the saved output; on a NaN
 * pre-activation it passes (torch's threshold_backward) where a mask taken from the saved output would zero it.  A non-finite
 * g propagates per element; the forward's row poison is not mimicked.
 * Supported (whvi_diag_apply_stacked_bwd_supported): log2d in [2, 12], J >= 1, J D <= 8192 (the forward's rule); anything else
 * returns WHVI_ERR_SIZE.  All pointers 16-byte aligned but g; grad_x, out and part must not overlap an input; S B < 2^32, S <= 65535;
 * n_slabs must be a slab count of B (ceil(B / ceil(B / n_slabs)) == n_slabs).  S B == 0 returns WHVI_OK without a launch. */
int whvi_diag_apply_stacked_bwd_supported(int32_t log2d, int64_t n_blocks);
int64_t whvi_diag_apply_stacked_bwd_slabs(int64_t S, int64_t B, int32_t log2d, int64_t n_blocks, int64_t n_cols);
int whvi_diag_apply_stacked_bwd_f32(void *grad_x, void *out, void *part, const void *g, const void *x, const void *s1,
                                    const void *s2, const void *u, const void *bias, int64_t S, int64_t B, int32_t log2d,
                                    int64_t n_blocks, int64_t n_cols, int64_t ld_g, int64_t n_slabs, int32_t flags, void *stream);

/* The two dense products either side of the square layer in a WHVI regression network, for all Monte-Carlo samples per launch,
 * as HBM-bound streams (f32; same dataflow as the reference's matrix products -- every product is formed, exact zeros of the
 * as-written weights included, so non-finite inputs propagate like in the dense product):
 *   whvi_small_k_apply_f32 : out[s, b, n] = sum_{c < K} x[b, c] * w[s, n, c] (+ bias[n]) (relu with WHVI_APPLY_RELU_OUT)
 *       `x_padded @ W.T` of WHVIStackedMatrix with a narrow input (src/weights.py:179-180,195-206; WHVILinear(3, 1024): K = 4,
 *       N = 1024).  x : (B, K) shared by all samples; w : (S, N, K); out : (S, B, N); K = 2^log2k in {4, 8}; N a multiple of 4
 *       with N / 4 = (a power of two <= 256) x (1 .. 4).  Fused multiply-adds in ascending c.
 *   whvi_row_dot_f32 : y[s, b] = sum_i x[s, b, i] * w[s, i] (+ bias[0])  (x through max(., 0) first with WHVI_APPLY_RELU_IN)
 *       `F.linear(x, w[None], bias)` of the transposed WHVIColumnMatrix (src/weights.py:239-251; WHVILinear(1024, 1)).
 *       x : (S, B, D); w : (S, D); y : (S, B); log2d in [2, 12].  Per-lane partial sums in ascending column order, then a
 *       butterfly over the wave's lanes: a different summation order than a GEMV's (same tolerance class). */
#define WHVI_APPLY_RELU_IN  1
#define WHVI_APPLY_RELU_OUT 2
int whvi_small_k_apply_f32(void *out, const void *x, const void *w, const void *bias, int64_t S, int64_t B, int64_t N,
                           int32_t log2k, int32_t flags, void *stream);
int whvi_row_dot_f32(void *y, const void *x, const void *w, const void *bias, int64_t S, int64_t B, int32_t log2d,
                     int32_t flags, void *stream);

/* The predictive pass of a WHVI regression network of the canonical shape -- WHVILinear(n_in, D), 1 .. 4 square
 * WHVILinear(D, D), WHVILinear(D, 1), an optional ReLU at every boundary -- for all Monte-Carlo samples in ONE launch that
 * keeps each row's hidden vector on chip (reads x, writes y; no (S, B, D) activation).  f32; per (s, b):
 *     h = first(x[b, :]; s) (+ b_in) (relu if bit 0 of relu)
 *     h = poison(h) * diag_m(s) + 0 (+ b_mid[m] if bit m of mid_bias) (relu if bit 1 + m of relu)    m = 0 .. n_mid - 1
 *     y[s, b] = row_dot(h, w_out[s]) (+ b_out[0])
 * with every stage the arithmetic of the launch it replaces, in the same order -- bit-identical to whvi_small_k_apply_f32 /
 * x * w, whvi_diag_apply_f32 (WHVI_DIAG_MEAN_PLUS) and whvi_row_dot_f32 in sequence:
 *   first = WHVI_MLP_FIRST_K4 / _K8 : x (B, K), w_in (S, D, K): fused multiply-adds in ascending c from +0 (stacked layer);
 *   first = WHVI_MLP_FIRST_COLUMN   : x (B, 1), w_in (S, D): the plain product x[b, 0] * w_in[s, n] (column layer);
 *   square layer m : s1, s2, b_mid (n_mid, D) rows m, u (n_mid, 1 + S, D) row block m -- mean row first, as whvi_diag_apply;
 *                    a row holding a non-finite value turns its other entries into NaN first (the dense product's rule);
 *   w_out (S, D), b_out one float or NULL; b_in D floats or NULL; b_mid may be NULL when mid_bias = 0.  A zero-filled bias
 *   is NOT the same as none: the add turns -0 into +0.
 * y (S, B) must not overlap any input; every pointer 16-byte aligned.  Supported: log2d in [6, 11], n_mid in [1, 4] and
 * the operands of one sample in 64 KiB of LDS: 4 * 2^log2d * (K + 2 + 2 n_mid) <= 65536 bytes (K = 1 for the column layer)
 * -- whvi_mlp_apply_supported(first, n_mid, log2d) returns 1 exactly then; otherwise the call returns WHVI_ERR_SIZE.
 * No allocation, no synchronisation: capture-safe. */
#define WHVI_MLP_FIRST_COLUMN 1
#define WHVI_MLP_FIRST_K4     4
#define WHVI_MLP_FIRST_K8     8
int whvi_mlp_apply_supported(int32_t first, int32_t n_mid, int32_t log2d);
int whvi_mlp_apply_f32(void *y, const void *x, int32_t first, const void *w_in, const void *b_in, int32_t n_mid,
                       const void *s1, const void *s2, const void *u, const void *b_mid, int32_t mid_bias,
                       const void *w_out, const void *b_out, int64_t S, int64_t B, int32_t log2d, int32_t relu,
                       void *stream);

/* Backward of whvi_mlp_apply_f32: from g = dL/dy (S, B) and the forward's operands (same arguments; b_out is not needed), the
 * gradients of every operand, without a saved activation.  Each row's hidden vectors are recomputed with the forward's
 * arithmetic (same ReLU masks, same poisoned rows), then the three-launch route's backward formulas run element by element:
 *     d = g * w_out;  at square layer m (last first): d = 0 where its fused ReLU's pre-activation, recomputed from the layer's
 *     input before the poison, has relu(z) <= 0 (NaN passes);  d = d * diag_m;  behind the first layer: d = 0 where h <= 0
 *     (column layer; NaN passes) or d = d * (h > 0) (stacked layer).
 *   grad_w_in  : (S, D, K) = sum_b d x[b, c]   (column layer: (S, D))
 *   grad_w_mid : (n_mid, S, D) = sum_b d_m h_{m-1}, the gradient w.r.t. each sample's diagonal (chain it to s1, s2, u as
 *                whvi_diag_apply_bwd's slots do)
 *   grad_w_out : (S, D) = sum_b g h_L
 *   grad_b     : (1 + n_mid) D + 1 floats: b_in (D), b_mid (n_mid rows of D), b_out (1), summed over samples and rows --
 *                written whatever the forward's bias pointers were
 *   grad_x     : (S, B, K) (column layer: (S, B, 1)) = sum_n d w_in[s, n, c], or NULL to skip; the caller sums over S
 *   work       : workspace of work_floats >= whvi_mlp_apply_bwd_workspace(S, B, first, n_mid, log2d) floats (WHVI_ERR_ARG
 *                otherwise).  Every block writes its partial sums there and a second, tiny launch inside the same call adds
 *                them in ascending slab and sample order: deterministic (bit-identical on every run), no atomics.
 * Supported: whvi_mlp_apply_supported's range with n_mid <= 2 and log2d <= 10 -- whvi_mlp_apply_bwd_supported(first, n_mid,
 * log2d) returns 1 exactly then, whvi_mlp_apply_bwd_workspace returns -1 otherwise.  Every argument check runs before any
 * launch.  No allocation, no synchronisation: capture-safe. */
int whvi_mlp_apply_bwd_supported(int32_t first, int32_t n_mid, int32_t log2d);
int64_t whvi_mlp_apply_bwd_workspace(int64_t S, int64_t B, int32_t first, int32_t n_mid, int32_t log2d);
int whvi_mlp_apply_bwd_f32(void *grad_w_in, void *grad_w_mid, void *grad_w_out, void *grad_b, void *grad_x, void *work,
                           int64_t work_floats, const void *g, const void *x, int32_t first, const void *w_in, const void *b_in,
                           int32_t n_mid, const void *s1, const void *s2, const void *u, const void *b_mid, int32_t mid_bias,
                           const void *w_out, int64_t S, int64_t B, int32_t log2d, int32_t relu, void *stream);

/* The one-launch passes with a choice of activation: whvi_mlp_apply_f32 / whvi_mlp_apply_bwd_f32 with `int32_t act, int32_t
 * act_bits` in place of `relu`.  act_bits has relu's layout (bit 0: behind the first layer, bit 1 + m: behind square layer m)
 * and says which boundaries carry the activation `act`:
 *   WHVI_MLP_ACT_RELU     relu(z), NaN passes -- exactly whvi_mlp_apply_f32 / whvi_mlp_apply_bwd_f32 with relu = act_bits
 *   WHVI_MLP_ACT_SIGMOID  y = 1.0f / (1.0f + expf(-z))   (ATen's float sigmoid: ocml expf, IEEE division)
 *                         backward d = (d * (1 - y)) * y  (torch's sigmoid_backward, on the recomputed y)
 *   WHVI_MLP_ACT_TANH     y = tanhf(z)                    (ocml)
 *                         backward d = d * (1 - y * y)    (torch's tanh_backward)
 * Non-finite values follow torch: sigmoid(+inf) = 1, sigmoid(-inf) = 0, tanh(+-inf) = +-1, NaN passes.  A smooth activation
 * sits where an nn.Sigmoid / nn.Tanh module sits on the three-launch route, before the next square layer's row poison (an
 * activated +-inf is finite and poisons nothing).  The backward recomputes y from the forward's arithmetic; no mask, no state.
 * Ranges, workspaces and every other rule are those of the ReLU entry points (whvi_mlp_apply_supported,
 * whvi_mlp_apply_bwd_supported, whvi_mlp_apply_bwd_workspace); an unknown act, or act_bits beyond the n_mid + 1 boundaries,
 * is WHVI_ERR_ARG.  Every argument check runs before any launch.  No allocation, no synchronisation: capture-safe. */
#define WHVI_MLP_ACT_RELU    1
#define WHVI_MLP_ACT_SIGMOID 2
#define WHVI_MLP_ACT_TANH    3
int whvi_mlp_apply_act_f32(void *y, const void *x, int32_t first, const void *w_in, const void *b_in, int32_t n_mid,
                           const void *s1, const void *s2, const void *u, const void *b_mid, int32_t mid_bias,
                           const void *w_out, const void *b_out, int64_t S, int64_t B, int32_t log2d, int32_t act,
                           int32_t act_bits, void *stream);
int whvi_mlp_apply_act_bwd_f32(void *grad_w_in, void *grad_w_mid, void *grad_w_out, void *grad_b, void *grad_x, void *work,
                               int64_t work_floats, const void *g, const void *x, int32_t first, const void *w_in,
                               const void *b_in, int32_t n_mid, const void *s1, const void *s2, const void *u,
                               const void *b_mid, int32_t mid_bias, const void *w_out, int64_t S, int64_t B, int32_t log2d,
                               int32_t act, int32_t act_bits, void *stream);

/* The predictive pass of a WHVI regression network whose square layers are FASTFOOD layers (WHVILinear(D, D, mode="fastfood"):
 * x -> s1 * H(g_k * H(s2 * x)), H the unnormalised Walsh-Hadamard transform) for all Monte-Carlo samples in ONE launch that
 * keeps each row's hidden vector on chip.  f32; per (s, b):
 *     h = first(x[b, :]; s) (+ b_in) (act if bit 0 of act_bits)                       -- as whvi_mlp_apply_f32
 *     h = s1[m] * H(g[m, s] * H(s2[m] * h)) (+ b_mid[m] if bit m of mid_bias) (act if bit 1 + m of act_bits)
 *     y[s, b] = row_dot(h, w_out[s]) (+ b_out[0])                                      -- as whvi_mlp_apply_f32
 * Each square layer repeats whvi_fused_shs_f32 (axis = COL, a = s1, b = g per sample, c = s2) and a separate bias add: the
 * result is bit-identical to that launch plus the add.  There is no row-poison rule: non-finite values propagate through the
 * butterflies.  first, x, w_in, b_in, w_out, b_out, act (WHVI_MLP_ACT_*) and act_bits are those of whvi_mlp_apply_act_f32;
 * s1, s2, b_mid (n_mid, D), g (n_mid, S, D).  y (S, B) must not overlap any input; every pointer 16-byte aligned.
 * Supported: log2d in [6, 11], n_mid in [1, 4] and the operands of one sample in 64 KiB of LDS:
 * 4 * 2^log2d * (K + 2 + 4 n_mid) <= 65536 bytes (K = 1 for the column layer) -- whvi_mlp_fastfood_apply_supported(first,
 * n_mid, log2d) returns 1 exactly then; otherwise the call returns WHVI_ERR_SIZE.  Every argument check runs before any
 * launch.  No allocation, no synchronisation: capture-safe. */
int whvi_mlp_fastfood_apply_supported(int32_t first, int32_t n_mid, int32_t log2d);
int whvi_mlp_fastfood_apply_f32(void *y, const void *x, int32_t first, const void *w_in, const void *b_in, int32_t n_mid,
                                const void *s1, const void *s2, const void *g, const void *b_mid, int32_t mid_bias,
                                const void *w_out, const void *b_out, int64_t S, int64_t B, int32_t log2d, int32_t act,
                                int32_t act_bits, void *stream);

/* Backward of whvi_mlp_fastfood_apply_f32: every parameter gradient of the network for all samples from g = dL/dy (S, B),
 * without any saved activation -- each block recomputes its rows' hidden vectors with the forward's arithmetic (the same
 * activation outputs and ReLU signs, bit for bit) and applies the batched route's backward formulas, last layer first:
 *     d = g * w_out;  at fastfood layer m, with its input h, t1 = H(s2 h), t2 = H(g_k t1) recomputed:  d = act'(.) d;
 *     grad_bias += d;  grad_s1 += d t2;  v = H(s1 d);  grad_g[k] += v t1;  w = H(g_k v);  grad_s2 += w h;  d = s2 w;
 *     behind the first layer d = act'(.) d, then the first layer's sums as whvi_mlp_apply_bwd_f32.
 *   act'(.) per boundary (act_bits), what the batched route runs there: sigmoid / tanh -- torch's formulas on the recomputed
 *     output; ReLU in front of the output layer (the row dot folds it) and behind a stacked first layer (its launch folds it):
 *     d = d * (out > 0); every other ReLU (an nn.ReLU module: behind a column first layer, between two fastfood layers):
 *     d = 0 where out <= 0, NaN passes.
 *   grad_w_in  : (S, D, K) = sum_b d x[b, c]   (column layer: (S, D))
 *   grad_s1, grad_s2 : (n_mid, D), summed over samples and rows
 *   grad_g     : (n_mid, S, D) = sum_b v t1, the gradient w.r.t. each sample's g_k
 *   grad_w_out : (S, D) = sum_b g h_L
 *   grad_b     : (1 + n_mid) D + 1 floats: b_in (D), b_mid (n_mid rows of D), b_out (1), summed over samples and rows --
 *                written whatever the forward's bias pointers were
 *   grad_x     : (S, B, K) (column layer: (S, B, 1)) = sum_n d w_in[s, n, c], or NULL to skip; the caller sums over S
 *   work       : workspace of work_floats >= whvi_mlp_fastfood_apply_bwd_workspace(S, B, first, n_mid, log2d) floats
 *                (WHVI_ERR_ARG otherwise).  Every block writes its partial sums there and a second, tiny launch inside the same
 *                call adds them in ascending slab and sample order: deterministic (bit-identical on every run), no atomics.
 * The other arguments are whvi_mlp_fastfood_apply_f32's (gk is its g).  No output and no part of the workspace may overlap an
 * input (WHVI_ERR_OVERLAP); every pointer 16-byte aligned.  Supported: whvi_mlp_fastfood_apply_supported's range with
 * n_mid <= 2 and log2d <= 10 -- whvi_mlp_fastfood_apply_bwd_supported(first, n_mid, log2d) returns 1 exactly then,
 * whvi_mlp_fastfood_apply_bwd_workspace returns -1 otherwise and the call WHVI_ERR_SIZE.  Every argument check runs before any
 * launch.  No allocation, no synchronisation: capture-safe. */
int whvi_mlp_fastfood_apply_bwd_supported(int32_t first, int32_t n_mid, int32_t log2d);
int64_t whvi_mlp_fastfood_apply_bwd_workspace(int64_t S, int64_t B, int32_t first, int32_t n_mid, int32_t log2d);
int whvi_mlp_fastfood_apply_bwd_f32(void *grad_w_in, void *grad_s1, void *grad_s2, void *grad_g, void *grad_w_out, void *grad_b,
                                    void *grad_x, void *work, int64_t work_floats, const void *g, const void *x, int32_t first,
                                    const void *w_in, const void *b_in, int32_t n_mid, const void *s1, const void *s2,
                                    const void *gk, const void *b_mid, int32_t mid_bias, const void *w_out, int64_t S, int64_t B,
                                    int32_t log2d, int32_t act, int32_t act_bits, void *stream);

/* whvi_reparam_kl_f32 with the eps draw inside the kernel: Philox4x32-10 + Box-Muller, one standard
 * normal per (matrix, sample, element), written to eps_out (J, S, D) for the backward pass / inspection.  The
 * generator state is three 64-bit words in DEVICE memory, state = {seed, launch offset, scratch (must be 0)}; the
 * kernel advances the offset itself when its last block finishes, so nothing about the draw is baked into the
 * launch: safe to capture in a hipGraph (every replay draws fresh eps).  One stream per state at a time.  The
 * stream of numbers is this library's own (not torch.randn's); for bit-level parity work inject eps through
 * whvi_reparam_kl_f32, which computes the same u / sigma / KL from a given eps.
 * The stream is a contract (tools/train_aux_ref.py restates it on the host, tests/test_train_aux_gpu.py holds the kernel to
 * it): the draw of a launch is a function of (seed, offset, j, k, i) alone.  For element i of matrix j, sample k:
 *     z = k / 8, q = k % 8, call = q / 4;
 *     counter = { i,  j << 16 | z,  low32(offset + call),  high32(offset + call) },  key = { low32(seed), high32(seed) };
 *     x[0..3] = Philox4x32-10(counter, key)   (multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85);
 *     the normals q % 4 = 0, 1, 2, 3 are  r(x0) cos t(x1),  r(x0) sin t(x1),  r(x2) cos t(x3),  r(x2) sin t(x3)  with
 *     u(x) = ((float)(x >> 8) + 0.5f) * 2^-24,  r = sqrtf(-2 logf(u)),  t = 6.283185307179586f * u.
 * So eight samples take TWO Philox calls of four normals each, and a launch moves the offset on by 2 whatever S is (S = 0
 * included): after n launches state = {seed, offset + 2 n, 0}.  u(x) maps onto (0, 1] -- the float32 sum rounds once x >> 8
 * reaches 2^23, and x >> 8 = 2^24 - 1 gives 1.0f, where r = 0 -- never onto 0, so the logarithm is finite. */
int whvi_reparam_kl_philox_f32(void *u, void *sigma, void *kl_part, void *eps_out, const void *g_mu,
                               const void *g_rho, void *state, int64_t J, int64_t S, int64_t D, float lambda_,
                               void *stream);

/* Backward of whvi_reparam_kl_f32 in one launch (closed form): grad_u (J, 1+S, D) and grad_kl (J) are the incoming
 * gradients (either may be NULL = zero), sigma the forward's saved output; writes grad_mu, grad_rho (J, D).
 * Replaces autograd over softplus / mul / kl_diag_normal (src/weights.py:43-64,82-83; src/utils.py:49-71).
 * The formulas assume that 1 / sigma is finite: below g_rho = -88.7 both 1 / sigma and expf(-g_rho) overflow and grad_rho
 * is inf * 0 = NaN where the exact value is finite (autograd over the op chain gives -inf there). */
int whvi_reparam_kl_bwd_f32(void *grad_mu, void *grad_rho, const void *grad_u, const void *grad_kl,
                            const void *g_mu, const void *g_rho, const void *eps, const void *sigma,
                            int64_t J, int64_t S, int64_t D, float lambda_, void *stream);

/* Gaussian mean negative log likelihood of MC predictions, replacing the per-output Python loop and
 * the elementwise chain of GaussianLikelihood.mnll_batch_estimate (src/likelihoods.py:18-29) by one reduction:
 *     part[b] = { scale * sum_b log N(y | y_hat, sigma^2),  sum_b z^2 },   z = (y - y_hat) / sigma
 * over three index dimensions size[0..2] (HOST arrays) with element strides yhat_stride / y_stride (y broadcasts
 * with stride 0 along the MC axis; order the dimensions by decreasing y_hat stride for coalesced reads);
 * mnll = sum_b part[b][0] with scale = -n / (m * n_mc); b < whvi_gauss_mnll_blocks(size[0]*size[1]*size[2]).
 * sigma is a DEVICE scalar (the learnable likelihood.sigma).  The backward writes
 *     grad_yhat = g * scale * (y - y_hat) / sigma^2   (same strides as y_hat),
 *     grad_sigma = g * scale * (sum z^2 - count) / sigma        with g = *grad_out (device scalar). */
int whvi_gauss_mnll_blocks(int64_t total);
int whvi_gauss_mnll_f32(void *part, const void *y, const void *y_hat, const void *sigma, const int64_t *size,
                        const int64_t *yhat_stride, const int64_t *y_stride, float scale, void *stream);
int whvi_gauss_mnll_bwd_f32(void *grad_yhat, void *grad_sigma, const void *grad_out, const void *part,
                            const void *y, const void *y_hat, const void *sigma, const int64_t *size,
                            const int64_t *yhat_stride, const int64_t *y_stride, float scale, void *stream);

/* Learning-rate schedule of the reference's experiments on the device (src/evaluation.py:25-26: LambdaLR with
 * lambda t: lambda0 * (1 + gamma * t) ** (-p); src/networks.py:80-81 steps it after every batch):
 *     if (advance) *t += 1;   *lr = (float)(base_lr * (lambda0 * pow(1 + gamma * *t, -p)))
 * t: DEVICE double (the step counter), lr: DEVICE float (the rate a capturable Adam reads).  One single-thread launch,
 * capture-safe; float64 arithmetic like LambdaLR's Python floats, one rounding to float32.  With several parameter
 * groups call it once per group, advance = 1 on the first only. */
int whvi_decay_lr_step(void *t, void *lr, double base_lr, double lambda0, double gamma, double p, int advance,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WHVI_HIP_H */
