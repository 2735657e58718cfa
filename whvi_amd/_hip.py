"""ctypes binding of ``libwhvi_hip.so`` (C ABI: ``include/whvi_hip.h``).

This is the only place the package touches the native library.  There is NO fallback: if the
library is missing or a call fails, a ``RuntimeError`` is raised -- a CUDA/HIP tensor is never
silently routed to a CPU implementation.

torch is used here for plumbing only: ``data_ptr()``, the current HIP stream and the device
guard.  The library links ``libamdhip64.so.7``; torch is imported first so that the HIP runtime
torch already loaded (same SONAME) is the one the kernels are registered with and the one whose
streams we launch on.
"""
import ctypes
import os
import threading

import torch  # noqa: F401  (must be loaded before the HIP library, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# The shipped loader reads NO environment: it loads the library built next to this file, or nothing.  (Measurement builds of
# the same library are loaded by the probes under tools/ by assigning LIB_PATH before the first call: tools/_tuning.py.)
LIB_PATH = os.path.join(_HERE, "libwhvi_hip.so")

AXIS_ROW, AXIS_COL = 0, 1
F32, F64, F16, I32, BF16 = 0, 1, 2, 3, 4

_DTYPE_CODE = {
    torch.float32: F32, torch.float64: F64, torch.float16: F16,
    torch.int32: I32, torch.bfloat16: BF16,
}
_DTYPE_SUFFIX = {
    torch.float32: "f32", torch.float64: "f64", torch.float16: "f16",
    torch.int32: "i32", torch.bfloat16: "bf16",
}

_lock = threading.Lock()
_lib = None


def _declare(lib):
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    lib.whvi_hip_abi_version.restype = ctypes.c_int
    lib.whvi_hip_abi_version.argtypes = []
    lib.whvi_last_error.restype = ctypes.c_char_p
    lib.whvi_last_error.argtypes = []
    lib.whvi_max_log2d.restype = ctypes.c_int
    lib.whvi_max_log2d.argtypes = [i32]
    lib.whvi_last_kernel.restype = ctypes.c_int
    lib.whvi_last_kernel.argtypes = [ctypes.c_char_p, i32]
    for sfx in ("f32", "f64", "f16", "bf16", "i32"):
        fn = getattr(lib, "whvi_fwht_" + sfx)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, i64, i32, vp]
    lib.whvi_fwht_ex.restype = ctypes.c_int
    lib.whvi_fwht_ex.argtypes = [vp, vp, i64, i32, i32, i32, vp]
    for sfx in ("f32", "f64"):
        fn = getattr(lib, "whvi_fused_shs_" + sfx)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, vp, i64, i32, i64, i64, i64, i32, vp]
        fn = getattr(lib, "whvi_fused_shs_ex_" + sfx)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, vp, i64, i32, i64, i64, i64, i32, i32, vp]
    for sfx in ("f16", "bf16"):                       # 16-bit activations, float32 scale vectors: the _ex form only
        fn = getattr(lib, "whvi_fused_shs_ex_" + sfx)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, vp, i64, i32, i64, i64, i64, i32, i32, vp]


def _declare_f3(lib):
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.whvi_reparam_kl_blocks.restype = ctypes.c_int
    lib.whvi_reparam_kl_blocks.argtypes = [i64]
    lib.whvi_reparam_kl_f32.restype = ctypes.c_int
    lib.whvi_reparam_kl_f32.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, ctypes.c_float, vp]
    lib.whvi_reparam_kl_philox_f32.restype = ctypes.c_int
    lib.whvi_reparam_kl_philox_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, ctypes.c_float, vp]
    lib.whvi_reparam_kl_bwd_f32.restype = ctypes.c_int
    lib.whvi_reparam_kl_bwd_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, ctypes.c_float, vp]
    p64 = ctypes.POINTER(ctypes.c_int64)
    lib.whvi_gauss_mnll_blocks.restype = ctypes.c_int
    lib.whvi_gauss_mnll_blocks.argtypes = [i64]
    lib.whvi_gauss_mnll_f32.restype = ctypes.c_int
    lib.whvi_gauss_mnll_f32.argtypes = [vp, vp, vp, vp, p64, p64, p64, ctypes.c_float, vp]
    lib.whvi_decay_lr_step.restype = ctypes.c_int
    lib.whvi_decay_lr_step.argtypes = [vp, vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int32, vp]
    lib.whvi_gauss_mnll_bwd_f32.restype = ctypes.c_int
    lib.whvi_gauss_mnll_bwd_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, p64, p64, p64, ctypes.c_float, vp]
    for sfx in ("f32", "f64"):
        fn = getattr(lib, "whvi_wbar_bwd_" + sfx)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, ctypes.c_int32, ctypes.c_int32, vp]
        fn = getattr(lib, "whvi_wbar_fwd_" + sfx)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, ctypes.c_int32, i64, i64, vp]
        fn = getattr(lib, "whvi_wbar_fwd_mean_" + sfx)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, i64, i64, i64, ctypes.c_int32, vp]
        fn = getattr(lib, "whvi_diag_apply_" + sfx)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, ctypes.c_int32, ctypes.c_int32, vp]
        fn = getattr(lib, "whvi_diag_apply_bwd_" + sfx)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, ctypes.c_int32, i64, ctypes.c_int32, vp]
    lib.whvi_diag_apply_stacked_supported.restype = ctypes.c_int
    lib.whvi_diag_apply_stacked_supported.argtypes = [ctypes.c_int32, i64]
    lib.whvi_diag_apply_stacked_f32.restype = ctypes.c_int
    lib.whvi_diag_apply_stacked_f32.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, ctypes.c_int32, i64, i64, i64, ctypes.c_int32, vp]
    lib.whvi_diag_apply_stacked_bwd_supported.restype = ctypes.c_int
    lib.whvi_diag_apply_stacked_bwd_supported.argtypes = [ctypes.c_int32, i64]
    lib.whvi_diag_apply_stacked_bwd_slabs.restype = i64
    lib.whvi_diag_apply_stacked_bwd_slabs.argtypes = [i64, i64, ctypes.c_int32, i64, i64]
    lib.whvi_diag_apply_stacked_bwd_f32.restype = ctypes.c_int
    lib.whvi_diag_apply_stacked_bwd_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, ctypes.c_int32, i64, i64, i64, i64,
                                                    ctypes.c_int32, vp]
    lib.whvi_small_k_apply_f32.restype = ctypes.c_int
    lib.whvi_small_k_apply_f32.argtypes = [vp, vp, vp, vp, i64, i64, i64, ctypes.c_int32, ctypes.c_int32, vp]
    lib.whvi_row_dot_f32.restype = ctypes.c_int
    lib.whvi_row_dot_f32.argtypes = [vp, vp, vp, vp, i64, i64, ctypes.c_int32, ctypes.c_int32, vp]
    i32 = ctypes.c_int32
    # the six network entry points share one operand block: x, first, w_in, b_in, n_mid, s1, s2, u / g, b_mid, mid_bias, w_out
    net = [vp, i32, vp, vp, i32, vp, vp, vp, vp, i32, vp]
    dims = [i64, i64, i32]                                              # S, B, log2d
    for name in ("mlp_apply", "mlp_fastfood_apply"):
        for query, restype, argtypes in (("_supported", ctypes.c_int, [i32, i32, i32]), ("_bwd_supported", ctypes.c_int, [i32, i32, i32]),
                                         ("_bwd_workspace", i64, [i64, i64, i32, i32, i32])):
            fn = getattr(lib, "whvi_" + name + query)
            fn.restype, fn.argtypes = restype, argtypes
    # (entry point, gradient outputs + workspace in front of the backward's work_floats and g, trailing act / act_bits words)
    for name, n_out, n_flags in (("mlp_apply", 6, 1), ("mlp_apply_act", 6, 2), ("mlp_fastfood_apply", 8, 2)):
        fwd, bwd = getattr(lib, "whvi_" + name + "_f32"), getattr(lib, "whvi_" + name + "_bwd_f32")
        fwd.restype = bwd.restype = ctypes.c_int
        fwd.argtypes = [vp] + net + [vp] + dims + [i32] * n_flags + [vp]           # y, ..., b_out, ..., stream
        bwd.argtypes = [vp] * n_out + [i64, vp] + net + dims + [i32] * n_flags + [vp]
    lib.whvi_fused_shs_bwd_supported.restype = ctypes.c_int
    lib.whvi_fused_shs_bwd_supported.argtypes = [i32]
    lib.whvi_fused_shs_bwd_workspace.restype = i64
    lib.whvi_fused_shs_bwd_workspace.argtypes = [i64, i64, i32]
    for sfx in ("f32", "f16", "bf16"):                # (16-bit: grad_x, grad_y and x; everything else float32)
        fn = getattr(lib, "whvi_fused_shs_bwd_" + sfx)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, vp]
    lib.whvi_fused_shs_stacked_supported.restype = ctypes.c_int
    lib.whvi_fused_shs_stacked_supported.argtypes = [i32, i64]
    lib.whvi_fused_shs_stacked_f32.restype = ctypes.c_int
    lib.whvi_fused_shs_stacked_f32.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, vp]
    lib.whvi_fused_shs_stacked16_supported.restype = ctypes.c_int
    lib.whvi_fused_shs_stacked16_supported.argtypes = [i32, i64]
    for fn in (lib.whvi_fused_shs_stacked_f16, lib.whvi_fused_shs_stacked_bf16):
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, vp]
    lib.whvi_fused_shs_stacked_layer_supported.restype = ctypes.c_int
    lib.whvi_fused_shs_stacked_layer_supported.argtypes = [i32, i64, i32]
    lib.whvi_fused_shs_stacked_layer_f32.restype = ctypes.c_int
    lib.whvi_fused_shs_stacked_layer_f32.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i64, i64, i32, vp]
    lib.whvi_fused_shs_stacked_layer16_supported.restype = ctypes.c_int
    lib.whvi_fused_shs_stacked_layer16_supported.argtypes = [i32, i64, i32]
    for fn in (lib.whvi_fused_shs_stacked_layer_f16, lib.whvi_fused_shs_stacked_layer_bf16):   # (16-bit: dst and src)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i64, i64, i32, vp]
    lib.whvi_fused_shs_stacked_bwd_supported.restype = ctypes.c_int
    lib.whvi_fused_shs_stacked_bwd_supported.argtypes = [i32, i64]
    lib.whvi_fused_shs_stacked_bwd_workspace.restype = i64
    lib.whvi_fused_shs_stacked_bwd_workspace.argtypes = [i64, i64, i32, i64]
    lib.whvi_fused_shs_stacked_bwd_f32.restype = ctypes.c_int
    lib.whvi_fused_shs_stacked_bwd_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, vp]
    lib.whvi_fused_shs_stacked_bwd16_supported.restype = ctypes.c_int
    lib.whvi_fused_shs_stacked_bwd16_supported.argtypes = [i32, i64]
    for fn in (lib.whvi_fused_shs_stacked_bwd_f16, lib.whvi_fused_shs_stacked_bwd_bf16):   # (16-bit: grad_x, grad_y and x)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, vp]
    lib.whvi_fused_shs_stacked_layer_bwd_supported.restype = ctypes.c_int
    lib.whvi_fused_shs_stacked_layer_bwd_supported.argtypes = [i32, i64, i32]
    lib.whvi_fused_shs_stacked_layer_bwd_workspace.restype = i64
    lib.whvi_fused_shs_stacked_layer_bwd_workspace.argtypes = [i64, i64, i32, i64, i32]
    lib.whvi_fused_shs_stacked_layer_bwd_f32.restype = ctypes.c_int
    lib.whvi_fused_shs_stacked_layer_bwd_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i64, i64,
                                                         i32, vp]
    lib.whvi_fused_shs_stacked_layer_bwd16_supported.restype = ctypes.c_int
    lib.whvi_fused_shs_stacked_layer_bwd16_supported.argtypes = [i32, i64, i32]
    for fn in (lib.whvi_fused_shs_stacked_layer_bwd_f16, lib.whvi_fused_shs_stacked_layer_bwd_bf16):   # (16-bit: grad_x, grad_y, y, x)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i64, i64, i32, vp]
    lib.whvi_stream_copy_probe.restype = ctypes.c_int
    lib.whvi_stream_copy_probe.argtypes = [vp, vp, i64, vp]
    lib.whvi_diag_apply_bwd_slabs.restype = ctypes.c_int64
    lib.whvi_diag_apply_bwd_slabs.argtypes = [ctypes.c_int32, i64, i64, ctypes.c_int32]
    lib.whvi_diag_apply_order.restype = ctypes.c_int32
    lib.whvi_diag_apply_order.argtypes = [ctypes.c_int32, i64, i64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    p32 = ctypes.POINTER(ctypes.c_int32)
    lib.whvi_fused_shs_plan.restype = ctypes.c_int32
    lib.whvi_fused_shs_plan.argtypes = [i32, i64, i32, i64, i64, i64, i32, i32, i32, i32, i32, i32, p32, p32, p32, p64]


def lib():
    """Load (once) and return the ctypes handle; raise loudly when it is not there."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"whvi_amd: native HIP library not found at {LIB_PATH}. Build it with "
                        "`python -c 'import __graft_entry__ as g; g.build()'` or "
                        "`make -C whvi_amd/csrc -j8`. There is no CPU fallback for GPU tensors.")
                handle = ctypes.CDLL(LIB_PATH)
                _declare(handle)
                _declare_f3(handle)
                if handle.whvi_hip_abi_version() != 1:
                    raise RuntimeError("whvi_amd: libwhvi_hip.so ABI version mismatch")
                _lib = handle
    return _lib


def is_built() -> bool:
    return os.path.exists(LIB_PATH)


def last_error() -> str:
    return lib().whvi_last_error().decode()


def last_kernel() -> str:
    """Demangled symbol of the kernel instantiation this thread's last FWHT / fused launch selected ("" before any)."""
    buf = ctypes.create_string_buffer(256)
    lib().whvi_last_kernel(buf, 256)
    return buf.value.decode()


def max_log2d(dtype: torch.dtype) -> int:
    return lib().whvi_max_log2d(_DTYPE_CODE[dtype])


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {last_error()}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t: torch.Tensor):
    """hipStream_t of torch's current stream on t's device (raw-handle fast path: no Stream object)."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class _OnDevice:
    """``with _OnDevice(dev):`` == ``with torch.cuda.device(dev):`` but free when dev is already current
    (the kernels launch on the calling thread's current device; the reference never sets it)."""
    __slots__ = ("dev", "ctx")

    def __init__(self, dev):
        self.dev, self.ctx = dev, None

    def __enter__(self):
        idx = self.dev.index
        if idx is not None and idx != torch.cuda.current_device():
            self.ctx = torch.cuda.device(self.dev)
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)


def _aligned(t: torch.Tensor) -> torch.Tensor:
    """Contiguous and 16-byte aligned view/copy of t (fresh torch allocations are 512-B aligned)."""
    t = t.contiguous()
    if t.data_ptr() % 16 != 0:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def _require_f32_on_one_device(what: str, dev, ops):
    if dev.type != "cuda" or any(t.device != dev or t.dtype != torch.float32 for t in ops):
        raise RuntimeError(f"{what}: float32 CUDA tensors on one device only")


FWHT_SIGNED_LANES = 1 << 23      # whvi_fwht_ex variant bit (include/whvi_hip.h): faster f32 / f64 streams, -0 results become +0


def fwht_rows(src: torch.Tensor, out: torch.Tensor = None, variant: int = None, signed_lanes: bool = False) -> torch.Tensor:
    """FWHT of every row of a contiguous (rows, D) device tensor.  ``out`` may alias ``src``
    (in place); by default a new tensor is returned and ``src`` is left untouched.  ``signed_lanes``: opt in to
    WHVI_FWHT_SIGNED_LANES (streams of f32 D = 512 .. 2048 / f64 D = 64 .. 2048: +1.7 %, the sign of a zero result is lost)."""
    if signed_lanes:
        variant = (variant or 0) | FWHT_SIGNED_LANES
    if src.device.type != "cuda":
        raise RuntimeError("X must be a CUDA tensor")
    if src.dim() != 2:
        raise RuntimeError("X must be two-dimensional")
    rows, d = src.shape
    if d < 1 or (d & (d - 1)) != 0:
        raise RuntimeError("n must be a power of 2")
    if src.dtype not in _DTYPE_CODE:
        raise RuntimeError(f"fwht: unsupported dtype {src.dtype} (float32/float64/float16/bfloat16/int32)")
    log2d = d.bit_length() - 1
    if out is None:
        src = _aligned(src)
        out = torch.empty_like(src, memory_format=torch.contiguous_format)
    else:
        if not (src.is_contiguous() and out.is_contiguous()):
            raise RuntimeError("fwht: src and out must be contiguous when out= is given")
        if out.shape != src.shape or out.dtype != src.dtype or out.device != src.device:
            raise RuntimeError("fwht: out must match src in shape, dtype and device")
    L = lib()
    with _OnDevice(src.device):
        if variant is None:
            rc = getattr(L, "whvi_fwht_" + _DTYPE_SUFFIX[src.dtype])(
                out.data_ptr(), src.data_ptr(), rows, log2d, _stream(src))
        else:
            rc = L.whvi_fwht_ex(out.data_ptr(), src.data_ptr(), rows, log2d,
                                _DTYPE_CODE[src.dtype], int(variant), _stream(src))
    _check(rc, "whvi_fwht")
    return out


def stream_copy_probe(src: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """whvi_stream_copy_probe: copy ``src`` (contiguous, a multiple of 16 bytes) with the transform kernels' streaming
    geometry and no arithmetic; ``out`` may be ``src`` (in place).  A measurement aid (bench.py: roofline.ceiling_measured)."""
    if src.device.type != "cuda" or not src.is_contiguous():
        raise RuntimeError("stream_copy_probe: contiguous CUDA tensor expected")
    if out is None:
        out = torch.empty_like(src)
    elif not out.is_contiguous() or out.numel() * out.element_size() != src.numel() * src.element_size() or out.device != src.device:
        raise RuntimeError("stream_copy_probe: out must match src")
    with _OnDevice(src.device):
        rc = lib().whvi_stream_copy_probe(out.data_ptr(), src.data_ptr(), src.numel() * src.element_size(), _stream(src))
    _check(rc, "whvi_stream_copy_probe")
    return out


FUSED_A_PER_SAMPLE, FUSED_C_PER_SAMPLE, FUSED_SRC_SHARED, FUSED_ONE_TRANSFORM = 1, 2, 4, 8
FUSED_RELU_IN, FUSED_RELU_OUT = 16, 32              # (fused_shs_stacked_layer, fused_shs_stacked_layer16, fused_shs_stacked_layer_bwd and fused_shs_stacked_layer_bwd16 only)
_HALF_DTYPES = (torch.float16, torch.bfloat16)


def fused_src_shared_supported(dtype: torch.dtype, d: int) -> bool:
    """Row lengths the shared-source form of ``whvi_fused_shs_*`` covers (rows of at least 64 sixteen-byte chunks)."""
    if dtype not in (torch.float32, torch.float64):
        return False                                  # 16-bit storage has the two-transform launch on its own rows only
    return fused_supported(dtype, d) and d * (4 if dtype == torch.float32 else 8) >= 1024


def fused_supported(dtype: torch.dtype, d: int) -> bool:
    """Row lengths ``whvi_fused_shs_*`` covers: one wavefront tile, D <= 8192 (f32) / 4096 (f64); float16 / bfloat16
    activations (float32 scale vectors, ``axis="col"`` with a source only) rows of one 16-byte chunk up to one tile,
    8 <= D <= 8192.  Longer rows have the plain transform only (``fwht_rows``: a block per row, then passes)."""
    if dtype == torch.float32:
        return 1 <= d <= 8192
    if dtype in _HALF_DTYPES:
        return 8 <= d <= 8192
    return dtype == torch.float64 and 1 <= d <= 4096


def fused_shs(src, a=None, b=None, c=None, *, axis: str = "col", n_samples: int = 1,
              sample_stride: int = 1, group_rows: int = 1, rows: int = None, d: int = None,
              dtype=None, device=None, out: torch.Tensor = None, a_per_sample: bool = False,
              c_per_sample: bool = False, src_shared: bool = False, one_transform: bool = False) -> torch.Tensor:
    """out[r] = a (.) FWHT(b_s (.) FWHT(c (.) src[r])) in ONE kernel (include/whvi_hip.h).

    ``src=None`` (axis="row", group_rows == d) synthesises the identity matrix per group, so
    with ``c = s2`` the input is ``torch.diag(s2)`` of src/weights.py:73 without reading HBM.
    ``src_shared`` (axis="col"): ``src`` is ``(sample_stride, d)`` -- ONE sample's rows, shared by all ``n_samples``
    samples -- and the result has ``n_samples * sample_stride`` rows in (sample, row) order (WHVI_FUSED_SRC_SHARED).
    ``one_transform`` (axis="col", ``c`` must be None): ``out[r] = a (.) FWHT(b_s (.) src[r])``, the second half alone.

    float16 / bfloat16 ``src`` (whvi_fused_shs_ex_f16 / _bf16): ``a``, ``b``, ``c`` are taken as float32, the arithmetic is
    float32 and the result is rounded to ``src``'s dtype ONCE, when it is stored -- the float32 pipeline on the upcast
    input, cast once.  ``axis="col"`` with a source only: ``axis="row"``, ``src=None``, ``src_shared`` and ``one_transform``
    raise.
    """
    ax = {"row": AXIS_ROW, "col": AXIS_COL}[axis]
    half = (src.dtype if src is not None else dtype) in _HALF_DTYPES
    if half:
        for refused, form in ((src is None, "src=None (identity source)"), (ax == AXIS_ROW, "axis='row'"),
                              (src_shared, "src_shared"), (one_transform, "one_transform")):
            if refused:
                raise RuntimeError(f"fused_shs: {form} has no float16 / bfloat16 form (float32 / float64 only)")
    if src is not None:
        if src.device.type != "cuda" or src.dim() != 2:
            raise RuntimeError("fused_shs: src must be a 2-D CUDA tensor")
        src = _aligned(src)
        rows, d = src.shape
        dtype, device = src.dtype, src.device
        if src_shared:
            if ax != AXIS_COL or rows != sample_stride or not fused_src_shared_supported(dtype, d):
                raise RuntimeError("fused_shs: src_shared needs axis='col', src of sample_stride rows and rows of >= 1 KiB")
            rows = n_samples * sample_stride
    if half:
        if not fused_supported(dtype, d):
            raise RuntimeError(f"fused_shs: {dtype} rows of {d} elements are outside the supported range 8 .. 8192")
    elif dtype not in (torch.float32, torch.float64):
        raise RuntimeError("fused_shs: float32 / float64 only (float16 / bfloat16: axis='col' with a source)")
    if d < 1 or (d & (d - 1)) != 0:
        raise RuntimeError("n must be a power of 2")
    log2d = d.bit_length() - 1

    def prep(v, n):
        if v is None:
            return None
        v = _aligned(v.to(device=device, dtype=torch.float32 if half else dtype).reshape(-1))
        if v.numel() != n:
            raise RuntimeError(f"fused_shs: scale vector has {v.numel()} elements, expected {n}")
        return v

    unit = group_rows if ax == AXIS_ROW else d
    a_ = prep(a, unit * (n_samples if a_per_sample else 1))
    b_ = prep(b, unit * n_samples)
    c_ = prep(c, unit * (n_samples if c_per_sample else 1))
    if one_transform and (c is not None or ax != AXIS_COL or src is None or not fused_src_shared_supported(dtype, d)):
        raise RuntimeError("fused_shs: one_transform needs axis='col', a source, c=None and rows of >= 1 KiB")
    flags = ((FUSED_A_PER_SAMPLE if a_per_sample else 0) | (FUSED_C_PER_SAMPLE if c_per_sample else 0) |
             (FUSED_SRC_SHARED if src_shared else 0) | (FUSED_ONE_TRANSFORM if one_transform else 0))
    if out is None:
        out = torch.empty((rows, d), dtype=dtype, device=device)
    elif not out.is_contiguous() or tuple(out.shape) != (rows, d) or out.dtype != dtype:
        raise RuntimeError("fused_shs: bad out tensor")
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    fn = getattr(lib(), "whvi_fused_shs_ex_" + _DTYPE_SUFFIX[dtype])
    with _OnDevice(device):
        rc = fn(out.data_ptr(), ptr(src), ptr(a_), ptr(b_), ptr(c_), rows, log2d, n_samples,
                sample_stride, group_rows, ax, flags, _stream(out))
    _check(rc, "whvi_fused_shs")
    return out


def fused_shs_plan(dtype_code: int, rows: int, log2d: int, n_samples: int = 1, sample_stride: int = 1, group_rows: int = 1,
                   axis: int = AXIS_COL, flags: int = 0, in_place: bool = False, src_null: bool = False, c_null: bool = False,
                   cus: int = 0):
    """whvi_fused_shs_plan: ``(rc, stage, nt, same_sample_blocks, grid)`` of the launch ``whvi_fused_shs_ex_<dtype>`` makes for
    these arguments on a device of ``cus`` compute units (0: the current device).  ``dtype_code``: ``F32`` / ``F64`` / ``F16`` /
    ``BF16``.  Launches nothing; with ``cus > 0`` no device is touched.  ``rc`` is the launch's error code where it refuses."""
    stage, nt, mode, grid = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1)
    rc = int(lib().whvi_fused_shs_plan(int(dtype_code), int(rows), int(log2d), int(n_samples), int(sample_stride), int(group_rows),
                                       int(axis), int(flags), int(bool(in_place)), int(bool(src_null)), int(bool(c_null)), int(cus),
                                       ctypes.byref(stage), ctypes.byref(nt), ctypes.byref(mode), ctypes.byref(grid)))
    return rc, stage.value, nt.value, mode.value, grid.value


def fused_shs_bwd_supported(dtype: torch.dtype, d: int) -> bool:
    """Row lengths the one-launch backward of the fused pipeline covers (``whvi_fused_shs_bwd_supported``): float32,
    64 <= D <= 4096."""
    if dtype != torch.float32 or d < 1 or (d & (d - 1)) != 0:
        return False
    return bool(lib().whvi_fused_shs_bwd_supported(d.bit_length() - 1))


def fused_shs_bwd16_supported(dtype: torch.dtype, d: int) -> bool:
    """Row lengths the one-launch backward covers on 16-bit activation streams (``whvi_fused_shs_bwd_f16 / _bf16``): float16 /
    bfloat16, 64 <= D <= 4096 -- the float32 launch's range (``whvi_fused_shs_bwd_supported`` serves both widths)."""
    if dtype not in _HALF_DTYPES or d < 1 or (d & (d - 1)) != 0:
        return False
    return bool(lib().whvi_fused_shs_bwd_supported(d.bit_length() - 1))


def fused_shs_bwd(grad_y: torch.Tensor, x: torch.Tensor, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, n_samples: int,
                  sample_stride: int, shared: bool = False, need_x: bool = True):
    """Backward of ``y = a * fwht(b_s * fwht(c * x))`` in one call (whvi_fused_shs_bwd_f32): ``(grad_x | None, grad_a (D),
    grad_b (S, D), grad_c (D))`` from ``grad_y`` ``(S * sample_stride, D)`` in (sample, row) order and the forward's operands.
    ``shared``: ``x`` is ``(sample_stride, D)``, read by every sample; ``grad_x`` still has ``S * sample_stride`` rows (the
    caller sums over samples).  ``need_x=False`` allocates and writes no ``grad_x``.  The workspace comes from torch's
    allocator, sized by ``whvi_fused_shs_bwd_workspace``.

    float16 / bfloat16 ``grad_y`` and ``x`` of one dtype with float32 ``a, b, c`` (whvi_fused_shs_bwd_f16 / _bf16): 6 * D bytes
    per row, float32 arithmetic on the exactly-upcast values, ``grad_x`` in that dtype (rounded once, when it is stored: the
    bits of ``fused_shs(grad_y, c, b, a)``) and float32 parameter gradients."""
    S, stride = int(n_samples), int(sample_stride)
    if grad_y.device.type != "cuda" or grad_y.dim() != 2:
        raise RuntimeError("fused_shs_bwd: grad_y must be a 2-D CUDA tensor")
    rows, d = grad_y.shape
    act = grad_y.dtype
    if act in _HALF_DTYPES:
        if x.dtype != act or x.device != grad_y.device:
            raise RuntimeError("fused_shs_bwd: grad_y and x must share one 16-bit dtype and device")
        _require_f32_on_one_device("fused_shs_bwd (16-bit activations: a, b, c)", grad_y.device, (a, b, c))
        if not fused_shs_bwd16_supported(act, d):
            raise RuntimeError(f"fused_shs_bwd: {act} rows of {d} elements are outside the supported range 64 .. 4096")
    else:
        _require_f32_on_one_device("fused_shs_bwd", grad_y.device, (grad_y, x, a, b, c))
        if not fused_shs_bwd_supported(torch.float32, d):
            raise RuntimeError(f"fused_shs_bwd: rows of {d} elements are outside the supported range 64 .. 4096")
    if (rows != S * stride or tuple(x.shape) != ((stride if shared else rows), d) or a.numel() != d or c.numel() != d
            or b.numel() != S * d):
        raise RuntimeError("fused_shs_bwd: operand shapes do not match (rows must be n_samples * sample_stride)")
    grad_y, x, a, b, c = (_aligned(t) for t in (grad_y, x, a.reshape(-1), b.reshape(-1), c.reshape(-1)))
    dev = grad_y.device
    grad_x = torch.empty((rows, d), dtype=act, device=dev) if need_x else None
    grad_a = torch.empty((d,), dtype=torch.float32, device=dev)
    grad_b = torch.empty((S, d), dtype=torch.float32, device=dev)
    grad_c = torch.empty((d,), dtype=torch.float32, device=dev)
    if rows == 0:
        return grad_x, grad_a.zero_(), grad_b.zero_(), grad_c.zero_()
    L = lib()
    log2d = d.bit_length() - 1
    n = int(L.whvi_fused_shs_bwd_workspace(S, stride, log2d))
    if n < 0:
        raise RuntimeError(f"whvi_fused_shs_bwd_workspace failed (code {n})")
    work = torch.empty((max(n, 16),), dtype=torch.uint8, device=dev)
    with _OnDevice(dev):
        fn = getattr(L, "whvi_fused_shs_bwd_" + _DTYPE_SUFFIX[act])
        rc = fn(None if grad_x is None else grad_x.data_ptr(), grad_a.data_ptr(), grad_b.data_ptr(), grad_c.data_ptr(),
                work.data_ptr(), grad_y.data_ptr(), x.data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr(), S, stride, log2d,
                FUSED_SRC_SHARED if shared else 0, _stream(grad_y))
    _check(rc, "whvi_fused_shs_bwd")
    return grad_x, grad_a, grad_b, grad_c


_F32_DTYPES = (torch.float32,)


def _stacked_fwd_rule(dtype, dtypes, d: int, n_blocks: int, has_bias: bool) -> bool:
    """The one support rule of the stacked forward launches (fused_stacked_layer_supported, fused_stacked_fwd.hpp, restated):
    the staged vectors and the bias are float32 whatever the activations are stored in."""
    if dtype not in dtypes or d < 1 or (d & (d - 1)) != 0:
        return False
    return 64 <= d <= 2048 and n_blocks >= 1 and (16 if has_bias else 12) * d * n_blocks <= 65536


def _fused_shs_stacked_fwd(name: str, dtypes, layer: bool, src, a, b, c, n_samples, sample_stride, shared, out,
                           bias=None, n_cols=None, relu_in=False, relu_out=False):
    """The one implementation behind ``fused_shs_stacked{,16}`` and ``fused_shs_stacked_layer{,16}``.  ``name``: the binding (the
    prefix of its messages; ``whvi_`` + ``name`` names the entry's errors); ``dtypes``: the activation dtypes it takes -- float32,
    or the 16-bit ones, whose chunk of 16 bytes is 8 columns and whose ``a, b, c, bias`` stay float32; ``layer``: the entry with
    the epilogue (``bias``, ``n_cols``, the two ReLUs and a pitched ``out``)."""
    half = dtypes is _HALF_DTYPES
    mult = 8 if half else 4                       # columns of a 16-byte chunk
    S, stride = int(n_samples), int(sample_stride)
    biases = () if bias is None else (bias,)
    if half:
        if src.device.type != "cuda" or src.dim() != 2 or src.dtype not in dtypes:
            raise RuntimeError(f"{name}: src must be a 2-D float16 / bfloat16 CUDA tensor")
        _require_f32_on_one_device(f"{name} (16-bit activations: a, b, c{', bias' if layer else ''})", src.device, (a, b, c) + biases)
    else:
        if src.device.type != "cuda" or src.dim() != 2:
            raise RuntimeError(f"{name}: src must be a 2-D CUDA tensor")
        _require_f32_on_one_device(name, src.device, (src, a, b, c) + biases)
    d = src.size(1)
    if a.dim() != 2 or a.size(1) != d:
        raise RuntimeError(f"{name}: a must be (n_blocks, D)")
    J = a.size(0)
    if not _stacked_fwd_rule(src.dtype, dtypes, d, J, bias is not None):
        if layer:
            raise RuntimeError(f"{name}: {J} blocks of {d} elements {'with' if bias is not None else 'without'} a bias "
                               "are outside the supported range (64 <= D <= 2048, (12 + 4 * bias) * D * n_blocks <= 65536)")
        raise RuntimeError(f"{name}: {J} blocks of {d} elements are outside the supported range "
                           "(64 <= D <= 2048, 12 * D * n_blocks <= 65536)")
    rows = S * stride
    n_cols = J * d if n_cols is None else int(n_cols)
    if src.size(0) != (stride if shared else rows) or tuple(c.shape) != (J, d) or tuple(b.shape) != (J, S, d) or \
            (bias is not None and bias.numel() != J * d):
        raise RuntimeError(f"{name}: operand shapes do not match (src rows must be n_samples * sample_stride, or "
                           f"sample_stride when shared; a, c (J, D); b (J, S, D){'; bias J * D elements' if layer else ''})")
    if n_cols % mult != 0 or not (J - 1) * d < n_cols <= J * d:
        raise RuntimeError(f"{name}: n_cols = {n_cols} must be a multiple of {mult} in ({(J - 1) * d}, {J * d}]")
    src, a, b, c = (_aligned(t) for t in (src, a, b, c))
    if bias is not None:
        bias = _aligned(bias)
    if out is None:
        out = torch.empty((rows, n_cols), dtype=src.dtype, device=src.device)
    else:
        ok = out.dim() == 2 and tuple(out.shape) == (rows, n_cols) and out.dtype == src.dtype and out.device == src.device
        if layer:                                 # its row stride is the launch's pitch
            ok = ok and (rows == 0 or (out.stride(1) == 1 and out.stride(0) % mult == 0 and out.stride(0) >= n_cols)) \
                and out.data_ptr() % 16 == 0
        else:
            ok = ok and out.is_contiguous()
        if not ok:
            raise RuntimeError(f"{name}: bad out tensor")
    if rows == 0:
        return out
    flags = (FUSED_SRC_SHARED if shared else 0) | (FUSED_RELU_IN if relu_in else 0) | (FUSED_RELU_OUT if relu_out else 0)
    fn = getattr(lib(), f"whvi_fused_shs_stacked_{'layer_' if layer else ''}{_DTYPE_SUFFIX[src.dtype]}")
    epilogue = (None if bias is None else bias.data_ptr(),) if layer else ()
    pitch = (n_cols, out.stride(0)) if layer else ()
    with _OnDevice(src.device):
        rc = fn(out.data_ptr(), src.data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr(), *epilogue, J, S, stride,
                d.bit_length() - 1, *pitch, flags, _stream(src))
    _check(rc, "whvi_" + name)
    return out


def fused_shs_stacked_supported(dtype: torch.dtype, d: int, n_blocks: int) -> bool:
    """Shapes the one-launch rectangular fastfood layer covers (``whvi_fused_shs_stacked_supported``, restated: no library
    needed): float32, 64 <= D <= 2048 and ``n_blocks >= 1`` triples of ``D`` floats within 64 KiB of LDS."""
    return _stacked_fwd_rule(dtype, _F32_DTYPES, d, n_blocks, False)


def fused_shs_stacked(src: torch.Tensor, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, n_samples: int, sample_stride: int,
                      shared: bool = False, out: torch.Tensor = None) -> torch.Tensor:
    """``out[r, j * D + n] = a[j, n] * fwht(b[j, s(r)] * fwht(c[j] * src[r]))[n]`` for all ``J`` blocks in ONE launch
    (whvi_fused_shs_stacked_f32): ``(n_samples * sample_stride, J * D)`` from ``src`` ``(n_samples * sample_stride, D)`` in
    (sample, row) order -- or ``(sample_stride, D)`` with ``shared``, read by every sample -- ``a, c`` ``(J, D)`` and ``b``
    ``(J, n_samples, D)``.  Block ``j`` of the result has the bits of ``fused_shs(src, a[j], b[j], c[j])``.  ``out``: a
    contiguous, 16-byte aligned ``(n_samples * sample_stride, J * D)`` float32 tensor to write instead of a new one."""
    return _fused_shs_stacked_fwd("fused_shs_stacked", _F32_DTYPES, False, src, a, b, c, n_samples, sample_stride, shared, out)


def fused_shs_stacked16_supported(dtype: torch.dtype, d: int, n_blocks: int) -> bool:
    """Shapes the one-launch rectangular fastfood layer covers on 16-bit activations (``whvi_fused_shs_stacked16_supported``,
    restated: no library needed): float16 / bfloat16, and ``fused_shs_stacked_supported``'s rule for the float32 vectors --
    64 <= D <= 2048 and ``n_blocks >= 1`` triples of ``D`` floats within 64 KiB of LDS."""
    return _stacked_fwd_rule(dtype, _HALF_DTYPES, d, n_blocks, False)


def fused_shs_stacked16(src: torch.Tensor, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, n_samples: int, sample_stride: int,
                        shared: bool = False, out: torch.Tensor = None) -> torch.Tensor:
    """``fused_shs_stacked`` for float16 / bfloat16 ``src`` with float32 ``a, c`` ``(J, D)`` and ``b`` ``(J, n_samples, D)``
    (whvi_fused_shs_stacked_f16 / _bf16): float32 arithmetic on the exactly-upcast input, the result in ``src``'s dtype,
    rounded ONCE when it is stored.  Block ``j`` has the bits of ``fused_shs(src, a[j], b[j], c[j])`` -- with ``shared``
    (``src`` ``(sample_stride, D)``, read by every sample) of that launch on ``src.repeat(n_samples, 1)``.  ``out``: a
    contiguous, 16-byte aligned ``(n_samples * sample_stride, J * D)`` tensor of ``src``'s dtype to write instead of a new one."""
    return _fused_shs_stacked_fwd("fused_shs_stacked16", _HALF_DTYPES, False, src, a, b, c, n_samples, sample_stride, shared, out)


def fused_shs_stacked_layer_supported(dtype: torch.dtype, d: int, n_blocks: int, has_bias: bool) -> bool:
    """Shapes the one-launch rectangular fastfood layer with its epilogue covers (``whvi_fused_shs_stacked_layer_supported``,
    restated: no library needed): float32, 64 <= D <= 2048 and ``n_blocks >= 1`` triples of ``D`` floats -- quadruples with a
    bias, which is staged with them -- within 64 KiB of LDS."""
    return _stacked_fwd_rule(dtype, _F32_DTYPES, d, n_blocks, has_bias)


def fused_shs_stacked_layer(src: torch.Tensor, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, n_samples: int,
                            sample_stride: int, bias: torch.Tensor = None, n_cols: int = None, relu_in: bool = False,
                            relu_out: bool = False, shared: bool = False, out: torch.Tensor = None) -> torch.Tensor:
    """``fused_shs_stacked`` with the layer's surroundings folded into the same launch (whvi_fused_shs_stacked_layer_f32):
    ``out[r, j * D + n] = act_out(a[j, n] * fwht(b[j, s(r)] * fwht(c[j] * act_in(src[r])))[n] + bias[j * D + n])`` for the first
    ``n_cols`` columns (default ``J * D``; a multiple of 4 that ends in the last block).  ``bias``: ``J * D`` floats of any shape, or
    None (no add at all); ``relu_in`` / ``relu_out``: ``torch.relu`` in front of / behind the layer.  Returns ``(rows, n_cols)``:
    a new contiguous tensor, or ``out`` -- a 2-D float32 tensor with ``stride(1) == 1``, ``stride(0) % 4 == 0``, ``stride(0) >=
    n_cols`` and a 16-byte aligned base, whose row stride is the launch's pitch; its columns past ``n_cols`` are not written."""
    return _fused_shs_stacked_fwd("fused_shs_stacked_layer", _F32_DTYPES, True, src, a, b, c, n_samples, sample_stride, shared, out,
                                  bias, n_cols, relu_in, relu_out)


def fused_shs_stacked_layer16_supported(dtype: torch.dtype, d: int, n_blocks: int, has_bias: bool) -> bool:
    """Shapes the one-launch rectangular fastfood layer with its epilogue covers on 16-bit activations
    (``whvi_fused_shs_stacked_layer16_supported``, restated: no library needed): float16 / bfloat16, and
    ``fused_shs_stacked_layer_supported``'s rule for the float32 vectors and bias -- 64 <= D <= 2048 and ``n_blocks >= 1`` triples
    of ``D`` floats, quadruples with a bias, within 64 KiB of LDS."""
    return _stacked_fwd_rule(dtype, _HALF_DTYPES, d, n_blocks, has_bias)


def fused_shs_stacked_layer16(src: torch.Tensor, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, n_samples: int,
                              sample_stride: int, bias: torch.Tensor = None, n_cols: int = None, relu_in: bool = False,
                              relu_out: bool = False, shared: bool = False, out: torch.Tensor = None) -> torch.Tensor:
    """``fused_shs_stacked_layer`` for float16 / bfloat16 ``src`` with float32 ``a, c`` ``(J, D)``, ``b`` ``(J, n_samples, D)`` and
    ``bias`` (``J * D`` floats of any shape, or None: no add at all) (whvi_fused_shs_stacked_layer_f16 / _bf16): float32
    arithmetic on the exactly-upcast input -- ``relu_in``, the three multiplies, the bias add and ``relu_out`` -- and the result
    in ``src``'s dtype, rounded ONCE when it is stored: ``fused_shs_stacked_layer(src.float(), ...).to(src.dtype)``.  The first
    ``n_cols`` columns are written (default ``J * D``; a multiple of 8 that ends in the last block).  Returns ``(rows, n_cols)``:
    a new contiguous tensor, or ``out`` -- a 2-D tensor of ``src``'s dtype with ``stride(1) == 1``, ``stride(0) % 8 == 0``,
    ``stride(0) >= n_cols`` and a 16-byte aligned base, whose row stride is the launch's pitch; its columns past ``n_cols`` are
    not written."""
    return _fused_shs_stacked_fwd("fused_shs_stacked_layer16", _HALF_DTYPES, True, src, a, b, c, n_samples, sample_stride, shared, out,
                                  bias, n_cols, relu_in, relu_out)


def fused_shs_stacked_bwd_supported(dtype: torch.dtype, d: int, n_blocks: int) -> bool:
    """Shapes the one-launch backward of the rectangular fastfood layer covers (``whvi_fused_shs_stacked_bwd_supported``,
    restated: no library needed): float32, 2 <= ``n_blocks`` <= 4 for 64 <= D <= 1024 and ``n_blocks`` = 2 at D = 2048."""
    if dtype != torch.float32 or d < 1 or (d & (d - 1)) != 0:
        return False
    return (64 <= d <= 1024 and 2 <= n_blocks <= 4) or (d == 2048 and n_blocks == 2)


def fused_shs_stacked_bwd(grad_y: torch.Tensor, x: torch.Tensor, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor,
                          n_samples: int, sample_stride: int, shared: bool = False, need_x: bool = True, grad_x: torch.Tensor = None):
    """Backward of ``fused_shs_stacked`` in one call (whvi_fused_shs_stacked_bwd_f32): ``(grad_x | None, grad_a (J, D), grad_b
    (J, S, D), grad_c (J, D))`` from ``grad_y`` ``(S * sample_stride, J * D)`` in (sample, row) order and the forward's operands
    ``x`` ``(S * sample_stride, D)``, ``a, c`` ``(J, D)``, ``b`` ``(J, S, D)``.  ``shared``: ``x`` is ``(sample_stride, D)``, read
    by every sample; ``grad_x`` still has ``S * sample_stride`` rows (the caller sums over samples).  ``need_x=False`` allocates
    and writes no ``grad_x``; ``grad_x``: a contiguous, 16-byte aligned ``(S * sample_stride, D)`` float32 tensor to write instead
    of a new one.  Block ``j``'s parameter gradients have the bits of ``fused_shs_bwd`` on the contiguous segment ``j`` of
    ``grad_y``, ``grad_x`` those of the per-block ``grad_x`` added in ascending ``j``.  The workspace comes from torch's
    allocator, sized by ``whvi_fused_shs_stacked_bwd_workspace``."""
    S, stride = int(n_samples), int(sample_stride)
    if grad_y.device.type != "cuda" or grad_y.dim() != 2:
        raise RuntimeError("fused_shs_stacked_bwd: grad_y must be a 2-D CUDA tensor")
    _require_f32_on_one_device("fused_shs_stacked_bwd", grad_y.device, (grad_y, x, a, b, c))
    if a.dim() != 2 or x.dim() != 2:
        raise RuntimeError("fused_shs_stacked_bwd: a must be (n_blocks, D) and x 2-D")
    J, d = a.shape
    if not fused_shs_stacked_bwd_supported(torch.float32, d, J):
        raise RuntimeError(f"fused_shs_stacked_bwd: {J} blocks of {d} elements are outside the supported range "
                           "(2 .. 4 blocks for 64 <= D <= 1024, 2 blocks at D = 2048)")
    rows = S * stride
    if (tuple(grad_y.shape) != (rows, J * d) or tuple(x.shape) != ((stride if shared else rows), d) or tuple(c.shape) != (J, d)
            or tuple(b.shape) != (J, S, d)):
        raise RuntimeError("fused_shs_stacked_bwd: operand shapes do not match (grad_y (n_samples * sample_stride, J * D); x the "
                           "same rows of D, or sample_stride rows when shared; a, c (J, D); b (J, S, D))")
    grad_y, x, a, b, c = (_aligned(t) for t in (grad_y, x, a, b, c))
    dev = grad_y.device
    if not need_x:
        grad_x = None
    elif grad_x is None:
        grad_x = torch.empty((rows, d), dtype=torch.float32, device=dev)
    elif not grad_x.is_contiguous() or tuple(grad_x.shape) != (rows, d) or grad_x.dtype != torch.float32 or grad_x.device != dev:
        raise RuntimeError("fused_shs_stacked_bwd: bad grad_x tensor")
    grad_a = torch.empty((J, d), dtype=torch.float32, device=dev)
    grad_b = torch.empty((J, S, d), dtype=torch.float32, device=dev)
    grad_c = torch.empty((J, d), dtype=torch.float32, device=dev)
    if rows == 0:
        return grad_x, grad_a.zero_(), grad_b.zero_(), grad_c.zero_()
    L = lib()
    log2d = d.bit_length() - 1
    n = int(L.whvi_fused_shs_stacked_bwd_workspace(S, stride, log2d, J))
    if n < 0:
        raise RuntimeError(f"whvi_fused_shs_stacked_bwd_workspace failed (code {n})")
    work = torch.empty((max(n, 16),), dtype=torch.uint8, device=dev)
    with _OnDevice(dev):
        rc = L.whvi_fused_shs_stacked_bwd_f32(None if grad_x is None else grad_x.data_ptr(), grad_a.data_ptr(), grad_b.data_ptr(),
                                              grad_c.data_ptr(), work.data_ptr(), grad_y.data_ptr(), x.data_ptr(), a.data_ptr(),
                                              b.data_ptr(), c.data_ptr(), J, S, stride, log2d, FUSED_SRC_SHARED if shared else 0,
                                              _stream(grad_y))
    _check(rc, "whvi_fused_shs_stacked_bwd")
    return grad_x, grad_a, grad_b, grad_c


def fused_shs_stacked_bwd16_supported(dtype: torch.dtype, d: int, n_blocks: int) -> bool:
    """Shapes the one-launch backward of the rectangular fastfood layer covers on 16-bit activations
    (``whvi_fused_shs_stacked_bwd16_supported``, restated: no library needed): float16 / bfloat16, and
    ``fused_shs_stacked_bwd_supported``'s rule for the float32 vectors -- 2 <= ``n_blocks`` <= 4 for 64 <= D <= 1024 and
    ``n_blocks`` = 2 at D = 2048."""
    if dtype not in _HALF_DTYPES or d < 1 or (d & (d - 1)) != 0:
        return False
    return (64 <= d <= 1024 and 2 <= n_blocks <= 4) or (d == 2048 and n_blocks == 2)


def fused_shs_stacked_bwd16(grad_y: torch.Tensor, x: torch.Tensor, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor,
                            n_samples: int, sample_stride: int, shared: bool = False, need_x: bool = True,
                            grad_x: torch.Tensor = None):
    """``fused_shs_stacked_bwd`` for float16 / bfloat16 ``grad_y`` and ``x`` of one dtype with float32 ``a, c`` ``(J, D)`` and
    ``b`` ``(J, S, D)`` (whvi_fused_shs_stacked_bwd_f16 / _bf16): ``(grad_x | None, grad_a (J, D), grad_b (J, S, D), grad_c
    (J, D))``, float32 arithmetic on the exactly-upcast values.  ``grad_x`` is in the activations' dtype and is rounded ONCE,
    after the last block: the float32 launch's ``grad_x`` on the upcasts, cast.  Block ``j``'s float32 parameter gradients have
    the bits of ``fused_shs_bwd`` (16-bit) on the contiguous segment ``j`` of ``grad_y``.  ``shared``, ``need_x``, ``grad_x``
    (a contiguous, 16-byte aligned ``(S * sample_stride, D)`` tensor of that dtype): as in ``fused_shs_stacked_bwd``.  The
    workspace comes from torch's allocator, sized by ``whvi_fused_shs_stacked_bwd_workspace``."""
    S, stride = int(n_samples), int(sample_stride)
    if grad_y.device.type != "cuda" or grad_y.dim() != 2 or grad_y.dtype not in _HALF_DTYPES:
        raise RuntimeError("fused_shs_stacked_bwd16: grad_y must be a 2-D float16 / bfloat16 CUDA tensor")
    act, dev = grad_y.dtype, grad_y.device
    if x.dtype != act or x.device != dev:
        raise RuntimeError("fused_shs_stacked_bwd16: grad_y and x must share one 16-bit dtype and device")
    _require_f32_on_one_device("fused_shs_stacked_bwd16 (16-bit activations: a, b, c)", dev, (a, b, c))
    if a.dim() != 2 or x.dim() != 2:
        raise RuntimeError("fused_shs_stacked_bwd16: a must be (n_blocks, D) and x 2-D")
    J, d = a.shape
    if not fused_shs_stacked_bwd16_supported(act, d, J):
        raise RuntimeError(f"fused_shs_stacked_bwd16: {J} blocks of {d} elements are outside the supported range "
                           "(2 .. 4 blocks for 64 <= D <= 1024, 2 blocks at D = 2048)")
    rows = S * stride
    if (tuple(grad_y.shape) != (rows, J * d) or tuple(x.shape) != ((stride if shared else rows), d) or tuple(c.shape) != (J, d)
            or tuple(b.shape) != (J, S, d)):
        raise RuntimeError("fused_shs_stacked_bwd16: operand shapes do not match (grad_y (n_samples * sample_stride, J * D); x the "
                           "same rows of D, or sample_stride rows when shared; a, c (J, D); b (J, S, D))")
    grad_y, x, a, b, c = (_aligned(t) for t in (grad_y, x, a, b, c))
    if not need_x:
        grad_x = None
    elif grad_x is None:
        grad_x = torch.empty((rows, d), dtype=act, device=dev)
    elif not grad_x.is_contiguous() or tuple(grad_x.shape) != (rows, d) or grad_x.dtype != act or grad_x.device != dev:
        raise RuntimeError("fused_shs_stacked_bwd16: bad grad_x tensor")
    grad_a = torch.empty((J, d), dtype=torch.float32, device=dev)
    grad_b = torch.empty((J, S, d), dtype=torch.float32, device=dev)
    grad_c = torch.empty((J, d), dtype=torch.float32, device=dev)
    if rows == 0:
        return grad_x, grad_a.zero_(), grad_b.zero_(), grad_c.zero_()
    L = lib()
    log2d = d.bit_length() - 1
    n = int(L.whvi_fused_shs_stacked_bwd_workspace(S, stride, log2d, J))
    if n < 0:
        raise RuntimeError(f"whvi_fused_shs_stacked_bwd_workspace failed (code {n})")
    work = torch.empty((max(n, 16),), dtype=torch.uint8, device=dev)
    fn = getattr(L, "whvi_fused_shs_stacked_bwd_" + _DTYPE_SUFFIX[act])
    with _OnDevice(dev):
        rc = fn(None if grad_x is None else grad_x.data_ptr(), grad_a.data_ptr(), grad_b.data_ptr(), grad_c.data_ptr(),
                work.data_ptr(), grad_y.data_ptr(), x.data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr(), J, S, stride, log2d,
                FUSED_SRC_SHARED if shared else 0, _stream(grad_y))
    _check(rc, "whvi_fused_shs_stacked_bwd16")
    return grad_x, grad_a, grad_b, grad_c


def fused_shs_stacked_layer_bwd_supported(dtype: torch.dtype, d: int, n_blocks: int, has_bias: bool) -> bool:
    """Shapes the one-launch backward of the rectangular fastfood layer with its epilogue covers
    (``whvi_fused_shs_stacked_layer_bwd_supported``, restated: no library needed): ``fused_shs_stacked_bwd_supported``'s rule,
    with or without a bias -- float32, 2 <= ``n_blocks`` <= 4 for 64 <= D <= 1024 and ``n_blocks`` = 2 at D = 2048."""
    if dtype != torch.float32 or d < 1 or (d & (d - 1)) != 0:
        return False
    return (64 <= d <= 1024 and 2 <= n_blocks <= 4) or (d == 2048 and n_blocks == 2)


def fused_shs_stacked_layer_bwd(grad_y: torch.Tensor, y, x: torch.Tensor, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor,
                                n_samples: int, sample_stride: int, n_cols: int = None, relu_in: bool = False,
                                relu_out: bool = False, shared: bool = False, need_x: bool = True, need_bias: bool = False,
                                grad_x: torch.Tensor = None):
    """Backward of ``fused_shs_stacked_layer`` in one call (whvi_fused_shs_stacked_layer_bwd_f32): ``(grad_x | None, grad_a
    (J, D), grad_b (J, S, D), grad_c (J, D), grad_bias (J * D) | None)`` from ``grad_y`` ``(S * sample_stride, n_cols)``, the
    forward's output ``y`` (the same shape and row stride; needed with ``relu_out`` only, ignored otherwise) and the forward's
    operands.  ``grad_y`` may be a view with ``stride(1) == 1``, ``stride(0) % 4 == 0`` and a 16-byte aligned base: its row stride is
    the launch's pitch and the columns past ``n_cols`` are never read.  The launch masks ``grad_y`` where ``y <= 0``
    (``relu_out``), treats the columns ``n_cols .. J * D - 1`` as zero, sums the masked gradient over the rows into ``grad_bias``
    (``need_bias``; zero from ``n_cols`` on), runs ``fused_shs_stacked_bwd``'s chain on ``relu(x)`` (``relu_in``) and masks
    ``grad_x`` where ``x <= 0`` -- no masked or padded copy, no ``relu(x)``.  ``grad_x, grad_a, grad_b, grad_c`` have the bits of
    those separate passes around ``fused_shs_stacked_bwd``; ``grad_bias`` is deterministic with a summation order of its own.
    ``shared``, ``need_x``, ``grad_x``: as in ``fused_shs_stacked_bwd``.  The workspace comes from torch's allocator, sized by
    ``whvi_fused_shs_stacked_layer_bwd_workspace``."""
    S, stride = int(n_samples), int(sample_stride)
    if grad_y.device.type != "cuda" or grad_y.dim() != 2:
        raise RuntimeError("fused_shs_stacked_layer_bwd: grad_y must be a 2-D CUDA tensor")
    if not relu_out:
        y = None
    elif y is None:
        raise RuntimeError("fused_shs_stacked_layer_bwd: relu_out needs the forward's output y")
    _require_f32_on_one_device("fused_shs_stacked_layer_bwd", grad_y.device, (grad_y, x, a, b, c) + (() if y is None else (y,)))
    if a.dim() != 2 or x.dim() != 2:
        raise RuntimeError("fused_shs_stacked_layer_bwd: a must be (n_blocks, D) and x 2-D")
    J, d = a.shape
    if not fused_shs_stacked_layer_bwd_supported(torch.float32, d, J, need_bias):
        raise RuntimeError(f"fused_shs_stacked_layer_bwd: {J} blocks of {d} elements are outside the supported range "
                           "(2 .. 4 blocks for 64 <= D <= 1024, 2 blocks at D = 2048)")
    rows = S * stride
    n_cols = grad_y.size(1) if n_cols is None else int(n_cols)
    if n_cols % 4 != 0 or not (J - 1) * d < n_cols <= J * d:
        raise RuntimeError(f"fused_shs_stacked_layer_bwd: n_cols = {n_cols} must be a multiple of 4 in ({(J - 1) * d}, {J * d}]")
    if (tuple(grad_y.shape) != (rows, n_cols) or tuple(x.shape) != ((stride if shared else rows), d) or tuple(c.shape) != (J, d)
            or tuple(b.shape) != (J, S, d) or (y is not None and tuple(y.shape) != (rows, n_cols))):
        raise RuntimeError("fused_shs_stacked_layer_bwd: operand shapes do not match (grad_y and y (n_samples * sample_stride, "
                           "n_cols); x the same rows of D, or sample_stride rows when shared; a, c (J, D); b (J, S, D))")

    def pitched(t):      # usable as it is (unit column stride, a pitch that is a multiple of 4, an aligned base), or a copy
        if rows > 1 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= n_cols and t.data_ptr() % 16 == 0:
            return t
        return _aligned(t)
    grad_y = pitched(grad_y)
    if y is not None:
        y = pitched(y)
        if rows > 1 and y.stride(0) != grad_y.stride(0):
            raise RuntimeError("fused_shs_stacked_layer_bwd: grad_y and y must have the same row stride")
    ld = grad_y.stride(0) if rows > 1 else n_cols
    x, a, b, c = (_aligned(t) for t in (x, a, b, c))
    dev = grad_y.device
    if not need_x:
        grad_x = None
    elif grad_x is None:
        grad_x = torch.empty((rows, d), dtype=torch.float32, device=dev)
    elif not grad_x.is_contiguous() or tuple(grad_x.shape) != (rows, d) or grad_x.dtype != torch.float32 or grad_x.device != dev:
        raise RuntimeError("fused_shs_stacked_layer_bwd: bad grad_x tensor")
    grad_a = torch.empty((J, d), dtype=torch.float32, device=dev)
    grad_b = torch.empty((J, S, d), dtype=torch.float32, device=dev)
    grad_c = torch.empty((J, d), dtype=torch.float32, device=dev)
    grad_bias = torch.empty((J * d,), dtype=torch.float32, device=dev) if need_bias else None
    if rows == 0:
        return grad_x, grad_a.zero_(), grad_b.zero_(), grad_c.zero_(), None if grad_bias is None else grad_bias.zero_()
    L = lib()
    log2d = d.bit_length() - 1
    n = int(L.whvi_fused_shs_stacked_layer_bwd_workspace(S, stride, log2d, J, 1 if need_bias else 0))
    if n < 0:
        raise RuntimeError(f"whvi_fused_shs_stacked_layer_bwd_workspace failed (code {n})")
    work = torch.empty((max(n, 16),), dtype=torch.uint8, device=dev)
    flags = (FUSED_SRC_SHARED if shared else 0) | (FUSED_RELU_IN if relu_in else 0) | (FUSED_RELU_OUT if relu_out else 0)
    with _OnDevice(dev):
        rc = L.whvi_fused_shs_stacked_layer_bwd_f32(None if grad_x is None else grad_x.data_ptr(), grad_a.data_ptr(),
                                                    grad_b.data_ptr(), grad_c.data_ptr(),
                                                    None if grad_bias is None else grad_bias.data_ptr(), work.data_ptr(),
                                                    grad_y.data_ptr(), None if y is None else y.data_ptr(), x.data_ptr(),
                                                    a.data_ptr(), b.data_ptr(), c.data_ptr(), J, S, stride, log2d, n_cols, ld, flags,
                                                    _stream(grad_y))
    _check(rc, "whvi_fused_shs_stacked_layer_bwd")
    return grad_x, grad_a, grad_b, grad_c, grad_bias


def fused_shs_stacked_layer_bwd16_supported(dtype: torch.dtype, d: int, n_blocks: int, has_bias: bool) -> bool:
    """Shapes the one-launch backward of the rectangular fastfood layer with its epilogue covers on 16-bit activations
    (``whvi_fused_shs_stacked_layer_bwd16_supported``, restated: no library needed): float16 / bfloat16, and
    ``fused_shs_stacked_bwd16_supported``'s rule, with or without a bias -- 2 <= ``n_blocks`` <= 4 for 64 <= D <= 1024 and
    ``n_blocks`` = 2 at D = 2048."""
    if dtype not in _HALF_DTYPES or d < 1 or (d & (d - 1)) != 0:
        return False
    return (64 <= d <= 1024 and 2 <= n_blocks <= 4) or (d == 2048 and n_blocks == 2)


def fused_shs_stacked_layer_bwd16(grad_y: torch.Tensor, y, x: torch.Tensor, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor,
                                  n_samples: int, sample_stride: int, n_cols: int = None, relu_in: bool = False,
                                  relu_out: bool = False, shared: bool = False, need_x: bool = True, need_bias: bool = False,
                                  grad_x: torch.Tensor = None):
    """``fused_shs_stacked_layer_bwd`` for float16 / bfloat16 ``grad_y``, ``y`` and ``x`` of one dtype with float32 ``a, c``
    ``(J, D)`` and ``b`` ``(J, S, D)`` (whvi_fused_shs_stacked_layer_bwd_f16 / _bf16): ``(grad_x | None, grad_a (J, D), grad_b
    (J, S, D), grad_c (J, D), grad_bias (J * D) | None)``, float32 arithmetic on the exactly-upcast values, the gradients of the
    vectors and of the bias in float32.  ``grad_y`` may be a view with ``stride(1) == 1``, ``stride(0) % 8 == 0`` and a 16-byte
    aligned base: its row stride is the launch's pitch and the columns past ``n_cols`` (a multiple of 8) are never read; ``y``
    must have the same row stride.  ``grad_x`` is in the activations' dtype and is rounded ONCE.  ``grad_x, grad_a, grad_b,
    grad_c`` have the bits of the separate 16-bit passes (``threshold_backward``, zero padding, ``relu(x)``, the mask on
    ``grad_x``) around ``fused_shs_stacked_bwd16``; ``grad_bias`` is the float32 column sum of the masked gradient, deterministic
    with a summation order of its own, zero from ``n_cols`` on.  The workspace comes from torch's allocator, sized by
    ``whvi_fused_shs_stacked_layer_bwd_workspace``."""
    S, stride = int(n_samples), int(sample_stride)
    if grad_y.device.type != "cuda" or grad_y.dim() != 2 or grad_y.dtype not in _HALF_DTYPES:
        raise RuntimeError("fused_shs_stacked_layer_bwd16: grad_y must be a 2-D float16 / bfloat16 CUDA tensor")
    act, dev = grad_y.dtype, grad_y.device
    if not relu_out:
        y = None
    elif y is None:
        raise RuntimeError("fused_shs_stacked_layer_bwd16: relu_out needs the forward's output y")
    if x.dtype != act or x.device != dev or (y is not None and (y.dtype != act or y.device != dev)):
        raise RuntimeError("fused_shs_stacked_layer_bwd16: grad_y, y and x must share one 16-bit dtype and device")
    _require_f32_on_one_device("fused_shs_stacked_layer_bwd16 (16-bit activations: a, b, c)", dev, (a, b, c))
    if a.dim() != 2 or x.dim() != 2:
        raise RuntimeError("fused_shs_stacked_layer_bwd16: a must be (n_blocks, D) and x 2-D")
    J, d = a.shape
    if not fused_shs_stacked_layer_bwd16_supported(act, d, J, need_bias):
        raise RuntimeError(f"fused_shs_stacked_layer_bwd16: {J} blocks of {d} elements are outside the supported range "
                           "(2 .. 4 blocks for 64 <= D <= 1024, 2 blocks at D = 2048)")
    rows = S * stride
    n_cols = grad_y.size(1) if n_cols is None else int(n_cols)
    if n_cols % 8 != 0 or not (J - 1) * d < n_cols <= J * d:
        raise RuntimeError(f"fused_shs_stacked_layer_bwd16: n_cols = {n_cols} must be a multiple of 8 in ({(J - 1) * d}, {J * d}]")
    if (tuple(grad_y.shape) != (rows, n_cols) or tuple(x.shape) != ((stride if shared else rows), d) or tuple(c.shape) != (J, d)
            or tuple(b.shape) != (J, S, d) or (y is not None and tuple(y.shape) != (rows, n_cols))):
        raise RuntimeError("fused_shs_stacked_layer_bwd16: operand shapes do not match (grad_y and y (n_samples * sample_stride, "
                           "n_cols); x the same rows of D, or sample_stride rows when shared; a, c (J, D); b (J, S, D))")

    def pitched(t):      # usable as it is (unit column stride, a pitch that is a multiple of 8, an aligned base), or a copy
        if rows > 1 and t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.stride(0) >= n_cols and t.data_ptr() % 16 == 0:
            return t
        return _aligned(t)
    grad_y = pitched(grad_y)
    if y is not None:
        y = pitched(y)
        if rows > 1 and y.stride(0) != grad_y.stride(0):
            raise RuntimeError("fused_shs_stacked_layer_bwd16: grad_y and y must have the same row stride")
    ld = grad_y.stride(0) if rows > 1 else n_cols
    x, a, b, c = (_aligned(t) for t in (x, a, b, c))
    if not need_x:
        grad_x = None
    elif grad_x is None:
        grad_x = torch.empty((rows, d), dtype=act, device=dev)
    elif not grad_x.is_contiguous() or tuple(grad_x.shape) != (rows, d) or grad_x.dtype != act or grad_x.device != dev:
        raise RuntimeError("fused_shs_stacked_layer_bwd16: bad grad_x tensor")
    grad_a = torch.empty((J, d), dtype=torch.float32, device=dev)
    grad_b = torch.empty((J, S, d), dtype=torch.float32, device=dev)
    grad_c = torch.empty((J, d), dtype=torch.float32, device=dev)
    grad_bias = torch.empty((J * d,), dtype=torch.float32, device=dev) if need_bias else None
    if rows == 0:
        return grad_x, grad_a.zero_(), grad_b.zero_(), grad_c.zero_(), None if grad_bias is None else grad_bias.zero_()
    L = lib()
    log2d = d.bit_length() - 1
    n = int(L.whvi_fused_shs_stacked_layer_bwd_workspace(S, stride, log2d, J, 1 if need_bias else 0))
    if n < 0:
        raise RuntimeError(f"whvi_fused_shs_stacked_layer_bwd_workspace failed (code {n})")
    work = torch.empty((max(n, 16),), dtype=torch.uint8, device=dev)
    flags = (FUSED_SRC_SHARED if shared else 0) | (FUSED_RELU_IN if relu_in else 0) | (FUSED_RELU_OUT if relu_out else 0)
    fn = getattr(L, "whvi_fused_shs_stacked_layer_bwd_" + _DTYPE_SUFFIX[act])
    with _OnDevice(dev):
        rc = fn(None if grad_x is None else grad_x.data_ptr(), grad_a.data_ptr(), grad_b.data_ptr(), grad_c.data_ptr(),
                None if grad_bias is None else grad_bias.data_ptr(), work.data_ptr(), grad_y.data_ptr(),
                None if y is None else y.data_ptr(), x.data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr(), J, S, stride, log2d,
                n_cols, ld, flags, _stream(grad_y))
    _check(rc, "whvi_fused_shs_stacked_layer_bwd16")
    return grad_x, grad_a, grad_b, grad_c, grad_bias


def reparam_kl(g_mu: torch.Tensor, g_rho: torch.Tensor, eps: torch.Tensor, lambda_: float):
    """One launch: (u (J, 1+S, D), sigma (J, D), kl (J,)) from g_mu, g_rho (J, D) and eps (J, S, D);
    see whvi_reparam_kl_f32 in include/whvi_hip.h."""
    if g_mu.device.type != "cuda" or g_mu.dtype != torch.float32:
        raise RuntimeError("reparam_kl: float32 CUDA tensors only")
    J, D = g_mu.shape
    S = eps.shape[1]
    g_mu, g_rho, eps = g_mu.contiguous(), g_rho.contiguous(), eps.contiguous()
    L = lib()
    nblk = (D + 255) // 256          # == whvi_reparam_kl_blocks(D)
    u = torch.empty((J, S + 1, D), dtype=torch.float32, device=g_mu.device)
    sigma = torch.empty((J, D), dtype=torch.float32, device=g_mu.device)
    part = torch.empty((J, nblk), dtype=torch.float32, device=g_mu.device)
    with _OnDevice(g_mu.device):
        rc = L.whvi_reparam_kl_f32(u.data_ptr(), sigma.data_ptr(), part.data_ptr(), g_mu.data_ptr(), g_rho.data_ptr(),
                                   eps.data_ptr() if S > 0 else None, J, S, D, float(lambda_), _stream(g_mu))
    _check(rc, "whvi_reparam_kl")
    return u, sigma, (part.sum(dim=1) if nblk > 1 else part[:, 0])


def new_rng_state(device, seed: int = None) -> torch.Tensor:
    """Device-resident generator state for ``reparam_kl_philox``: int64 [seed, launch offset, scratch].  Without an
    explicit seed one is drawn from torch's default CPU generator, so ``torch.manual_seed`` makes runs repeatable."""
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    return torch.tensor([int(seed), 0, 0], dtype=torch.int64, device=device)


def reparam_kl_philox(g_mu: torch.Tensor, g_rho: torch.Tensor, n_samples: int, lambda_: float, state: torch.Tensor):
    """One launch, eps drawn in the kernel: (u (J, 1+S, D), sigma (J, D), kl (J,), eps (J, S, D)); see
    whvi_reparam_kl_philox_f32 in include/whvi_hip.h.  ``state`` comes from ``new_rng_state`` and is advanced in place."""
    if g_mu.device.type != "cuda" or g_mu.dtype != torch.float32:
        raise RuntimeError("reparam_kl_philox: float32 CUDA tensors only")
    if state.dtype != torch.int64 or state.numel() < 3 or state.device != g_mu.device or not state.is_contiguous():
        raise RuntimeError("reparam_kl_philox: state must be a contiguous int64 tensor of 3 words on the same device")
    J, D = g_mu.shape
    S = int(n_samples)
    g_mu, g_rho = g_mu.contiguous(), g_rho.contiguous()
    L = lib()
    nblk = (D + 255) // 256
    dev = g_mu.device
    u = torch.empty((J, S + 1, D), dtype=torch.float32, device=dev)
    sigma = torch.empty((J, D), dtype=torch.float32, device=dev)
    part = torch.empty((J, nblk), dtype=torch.float32, device=dev)
    eps = torch.empty((J, S, D), dtype=torch.float32, device=dev)
    with _OnDevice(dev):
        rc = L.whvi_reparam_kl_philox_f32(u.data_ptr(), sigma.data_ptr(), part.data_ptr(), eps.data_ptr() if S > 0 else None,
                                          g_mu.data_ptr(), g_rho.data_ptr(), state.data_ptr(), J, S, D, float(lambda_),
                                          _stream(g_mu))
    _check(rc, "whvi_reparam_kl_philox")
    return u, sigma, (part.sum(dim=1) if nblk > 1 else part[:, 0]), eps


def wbar_bwd_supported(dtype: torch.dtype, d: int) -> bool:
    """Shapes the one-launch backward covers (rows of one 16-byte chunk up to one wavefront tile)."""
    if dtype == torch.float32:
        return 4 <= d <= 8192
    return dtype == torch.float64 and 2 <= d <= 4096


def wbar_fwd(s1: torch.Tensor, u: torch.Tensor, s2: torch.Tensor, rows: int = None, base: torch.Tensor = None,
             first: int = 0, count: int = None):
    """One launch: W (J, S, R, D) with W[j,k] = the first R rows of S1_j fwht(diag(u[j, first + k]) fwht(diag(s2_j))),
    k < S = ``count`` (default: all rows of ``u`` from ``first`` on), plus ``base`` (J, R, D) when given; see
    whvi_wbar_fwd_f32 in include/whvi_hip.h."""
    if u.device.type != "cuda" or u.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("wbar_fwd: float32 / float64 CUDA tensors only")
    J, G, D = u.shape
    S = G - first if count is None else int(count)
    R = D if rows is None else int(rows)
    if first < 0 or S < 0 or first + S > G:
        raise RuntimeError("wbar_fwd: rows first .. first + count do not fit u")
    if tuple(s1.shape) != (J, D) or tuple(s2.shape) != (J, D) or (base is not None and tuple(base.shape) != (J, R, D)):
        raise RuntimeError("wbar_fwd: operand shapes do not match u")
    if not (s1.dtype == s2.dtype == u.dtype) or (base is not None and base.dtype != u.dtype):
        raise RuntimeError("wbar_fwd: operand dtypes do not match u")
    s1, u, s2 = s1.contiguous(), u.contiguous(), s2.contiguous()
    base = None if base is None else base.contiguous()
    out = torch.empty((J, S, R, D), dtype=u.dtype, device=u.device)
    fn = getattr(lib(), "whvi_wbar_fwd_" + _DTYPE_SUFFIX[u.dtype])
    with _OnDevice(u.device):
        rc = fn(out.data_ptr(), s1.data_ptr(), u.data_ptr(), s2.data_ptr(), None if base is None else base.data_ptr(),
                J, S, R, D.bit_length() - 1, G, int(first), _stream(u))
    _check(rc, "whvi_wbar_fwd")
    return out


# results up to this size take the one-launch mean + sample form (whvi_wbar_fwd_mean); beyond it the two-launch form wins
# (half the arithmetic per byte written once the write stream itself is the bound).  Measured, interleaved, HIP events
# (tools/probe_wbar_mean.py, profiles/r03/wbar_mean_one_vs_two_launches.log): 256 matrices of D = 4 x 16 samples 7.5 vs
# 16.3 us, D = 512 x 32 (32 MiB, config 2) 12.9 vs 16.8 us; D = 1024 x 16 (64 MiB) 21.1 vs 17.1, 128 MiB 35 vs 25
WBAR_INLINE_MEAN_MAX_BYTES = 48 << 20


def wbar_fwd_mean(s1: torch.Tensor, u: torch.Tensor, s2: torch.Tensor, rows: int = None, inline: bool = None):
    """W (J, S, R, D) with W[j,k] = w_bar(u[j,0]) + w_bar(u[j,1+k]) for u (J, 1 + S, D) -- src/weights.py:93.  One launch
    computing both terms (``whvi_wbar_fwd_mean``) for cache-resident results, otherwise the mean matrix once and every
    sample's matrix with the mean added in its epilogue (two launches of ``whvi_wbar_fwd``).  Same bits either way;
    ``inline`` forces the choice (tests, A/B)."""
    if u.device.type != "cuda" or u.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("wbar_fwd_mean: float32 / float64 CUDA tensors only")
    J, G, D = u.shape
    S, R = G - 1, (D if rows is None else int(rows))
    if S < 0 or tuple(s1.shape) != (J, D) or tuple(s2.shape) != (J, D) or not (s1.dtype == s2.dtype == u.dtype):
        raise RuntimeError("wbar_fwd_mean: operands do not match u")
    fits = D <= (4096 if u.dtype == torch.float32 else 2048)      # two 64-register tiles per wave
    if inline is None:
        inline = fits and J * S * R * D * u.element_size() <= WBAR_INLINE_MEAN_MAX_BYTES
    elif inline and not fits:
        raise RuntimeError("wbar_fwd_mean: rows this long have the two-launch form only")
    if not inline:
        mean = wbar_fwd(s1, u, s2, R, first=0, count=1)                        # (J, 1, R, D): w_bar(g_mu), once
        return wbar_fwd(s1, u, s2, R, base=mean.view(J, R, D), first=1)        # + w_bar(g_sigma * eps_k), per sample
    s1, u, s2 = s1.contiguous(), u.contiguous(), s2.contiguous()
    out = torch.empty((J, S, R, D), dtype=u.dtype, device=u.device)
    fn = getattr(lib(), "whvi_wbar_fwd_mean_" + _DTYPE_SUFFIX[u.dtype])
    with _OnDevice(u.device):
        rc = fn(out.data_ptr(), s1.data_ptr(), u.data_ptr(), s2.data_ptr(), J, S, R, D.bit_length() - 1, _stream(u))
    _check(rc, "whvi_wbar_fwd_mean")
    return out


def wbar_bwd(grad_w: torch.Tensor, s1: torch.Tensor, u: torch.Tensor, s2: torch.Tensor, mean: bool = False,
             no_lds: bool = False, tiles: str = None):
    """One launch: a (3, J, U, D) tensor [grad_u, part_s1, part_s2] from grad_w (J, S, R, D), s1 / s2 (J, D) and
    u (J, U, D), U = S -- or 1 + S with ``mean`` (W[j,k] = w_bar(u[j,0]) + w_bar(u[j,1+k]); slot 0 of the result is
    then left for the caller's sum over slots 1..S).  Entries i >= R are zero.  ``no_lds`` (tuning / cross-check):
    WHVI_WBAR_NO_LDS, the DPP butterfly network instead of the LDS-staged one; ``tiles`` = "small" / "big" forces or
    forbids the quarter-size tiles of small problems.  See whvi_wbar_bwd_f32."""
    if grad_w.device.type != "cuda" or grad_w.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("wbar_bwd: float32 / float64 CUDA tensors only")
    J, S, R, D = grad_w.shape
    U = S + 1 if mean else S
    if tuple(u.shape) != (J, U, D) or tuple(s1.shape) != (J, D) or tuple(s2.shape) != (J, D):
        raise RuntimeError("wbar_bwd: operand shapes do not match grad_w")
    if not (u.dtype == s1.dtype == s2.dtype == grad_w.dtype):
        raise RuntimeError("wbar_bwd: operand dtypes do not match grad_w")
    grad_w, s1, u, s2 = grad_w.contiguous(), s1.contiguous(), u.contiguous(), s2.contiguous()
    alloc = torch.empty if R == D else torch.zeros
    out = alloc((3, J, U, D), dtype=grad_w.dtype, device=grad_w.device)
    fn = getattr(lib(), "whvi_wbar_bwd_" + _DTYPE_SUFFIX[grad_w.dtype])
    with _OnDevice(grad_w.device):
        rc = fn(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), grad_w.data_ptr(), s1.data_ptr(),
                u.data_ptr(), s2.data_ptr(), J, S, R, D.bit_length() - 1, (1 if mean else 0) | (2 if no_lds else 0) | {None: 0, "small": 4, "big": 8}[tiles],
                _stream(grad_w))
    _check(rc, "whvi_wbar_bwd")
    return out


DIAG_X_SHARED, DIAG_MEAN_PLUS, DIAG_RELU_IN, DIAG_RELU_OUT = 1, 2, 4, 8
DIAG_TUNE_NT, DIAG_TUNE_CACHED, DIAG_TUNE_PLAIN_ORDER = 16, 32, 64      # tuning / cross-check flags (include/whvi_hip.h)
DIAG_ORDER_PLAIN, DIAG_ORDER_XCD, DIAG_ORDER_SAMPLE_FASTEST = 0, 1, 2    # whvi_diag_apply_order


def diag_apply_supported(dtype: torch.dtype, d: int) -> bool:
    """Row lengths ``whvi_diag_apply_*`` covers: one 16-byte chunk up to one 64-register wavefront tile."""
    if dtype == torch.float32:
        return 4 <= d <= 4096 and (d & (d - 1)) == 0
    return dtype == torch.float64 and 2 <= d <= 2048 and (d & (d - 1)) == 0


def diag_apply_order(dtype: torch.dtype, n_samples: int, batch: int, d: int, flags: int = 0, in_place: bool = False) -> int:
    """whvi_diag_apply_order: the block order (``DIAG_ORDER_*``) of the launch ``whvi_diag_apply`` makes for ``n_samples`` x
    ``batch`` rows of ``d`` elements with ``flags`` (``DIAG_X_SHARED`` and the tuning flags decide it).  Launches nothing."""
    if dtype not in (torch.float32, torch.float64):
        raise RuntimeError("diag_apply_order: float32 / float64 only")
    rc = int(lib().whvi_diag_apply_order(_DTYPE_CODE[dtype], int(n_samples), int(batch), int(d).bit_length() - 1, int(flags),
                                         1 if in_place else 0))
    if rc < 0 or d & (d - 1):
        raise RuntimeError(f"diag_apply_order: unsupported arguments (code {rc})")
    return rc


def _diag_operands(x, s1, s2, u, n_samples, mean_plus, what, relu_in=False, relu_out=False):
    if x.device.type != "cuda" or x.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"{what}: float32 / float64 CUDA tensors only")
    D = x.shape[-1]
    if not diag_apply_supported(x.dtype, D):
        raise RuntimeError(f"{what}: D = {D} is outside the supported range for {x.dtype}")
    S = int(n_samples)
    if x.dim() == 3 and x.shape[0] == S:
        shared, B = False, x.shape[1]
    elif x.dim() == 2:
        shared, B = True, x.shape[0]
    else:
        raise RuntimeError(f"{what}: x must be (n_samples, batch, D) or (batch, D)")
    U = S + (1 if mean_plus else 0)
    if tuple(u.shape) != (U, D) or tuple(s1.shape) != (D,) or tuple(s2.shape) != (D,):
        raise RuntimeError(f"{what}: operand shapes do not match x (u must be ({U}, {D}))")
    if not (u.dtype == s1.dtype == s2.dtype == x.dtype):
        raise RuntimeError(f"{what}: operand dtypes do not match x")
    flags = ((DIAG_X_SHARED if shared else 0) | (DIAG_MEAN_PLUS if mean_plus else 0) | (DIAG_RELU_IN if relu_in else 0) |
             (DIAG_RELU_OUT if relu_out else 0))
    return S, B, D, shared, flags


def diag_apply(x: torch.Tensor, s1: torch.Tensor, s2: torch.Tensor, u: torch.Tensor, bias: torch.Tensor = None, *,
               n_samples: int, mean_plus: bool = True, out: torch.Tensor = None, tune: int = 0, relu_in: bool = False,
               relu_out: bool = False) -> torch.Tensor:
    """One launch: ``out[k] = x[(k)] * (wd(u[0]) + wd(u[1 + k])) + bias`` -- ``h @ (w_bar(g_mu) + w_bar(g_sigma eps_k)).T``
    of src/weights.py:87-93 for all MC samples without the matrices; see whvi_diag_apply_f32 in include/whvi_hip.h.
    ``x``: (S, B, D) or a shared (B, D); ``u``: (1 + S, D), or (S, D) with ``mean_plus=False``; returns (S, B, D).
    ``relu_in`` / ``relu_out``: an ``nn.ReLU`` in front of / behind the layer fused into the launch (WHVI_DIAG_RELU_*)."""
    S, B, D, shared, flags = _diag_operands(x, s1, s2, u, n_samples, mean_plus, "diag_apply", relu_in, relu_out)
    x, s1, s2, u = _aligned(x), _aligned(s1), _aligned(s2), _aligned(u)
    if bias is not None:
        if bias.numel() != D or bias.dtype != x.dtype:
            raise RuntimeError("diag_apply: bias must hold D elements of x's dtype")
        bias = _aligned(bias.reshape(-1))
    if out is None:
        out = torch.empty((S, B, D), dtype=x.dtype, device=x.device)
    elif not out.is_contiguous() or tuple(out.shape) != (S, B, D) or out.dtype != x.dtype or out.data_ptr() % 16:
        raise RuntimeError("diag_apply: bad out tensor")
    fn = getattr(lib(), "whvi_diag_apply_" + _DTYPE_SUFFIX[x.dtype])
    with _OnDevice(x.device):
        rc = fn(out.data_ptr(), x.data_ptr(), s1.data_ptr(), s2.data_ptr(), u.data_ptr(),
                None if bias is None else bias.data_ptr(), S, B, D.bit_length() - 1, flags | int(tune), _stream(x))
    _check(rc, "whvi_diag_apply")
    return out


def diag_apply_bwd(grad_out: torch.Tensor, x: torch.Tensor, s1: torch.Tensor, s2: torch.Tensor, u: torch.Tensor, *,
                   n_samples: int, mean_plus: bool = True, need_grad_x: bool = True, tune: int = 0, bias: torch.Tensor = None,
                   relu_in: bool = False, relu_out: bool = False):
    """Backward of ``diag_apply`` in one call: ``(grad_x (S, B, D) or None, out (4, U, D))`` with the rows of ``out`` as
    whvi_diag_apply_bwd_f32 documents them (slot 0 dL/du, 1 / 2 the per-sample shares of dL/ds1 / dL/ds2, 3 of dL/dbias;
    with ``mean_plus`` row 0 is left for the caller's sum over rows 1 ..)."""
    S, B, D, shared, flags = _diag_operands(x, s1, s2, u, n_samples, mean_plus, "diag_apply_bwd", relu_in, relu_out)
    if bias is not None:
        bias = _aligned(bias.reshape(-1))
    if tuple(grad_out.shape) != (S, B, D) or grad_out.dtype != x.dtype:
        raise RuntimeError("diag_apply_bwd: grad_out must be (n_samples, batch, D) of x's dtype")
    grad_out, x, s1, s2, u = _aligned(grad_out), _aligned(x), _aligned(s1), _aligned(s2), _aligned(u)
    L = lib()
    log2d = D.bit_length() - 1
    U = u.shape[0]
    out = torch.empty((4, U, D), dtype=x.dtype, device=x.device)
    grad_x = torch.empty((S, B, D), dtype=x.dtype, device=x.device) if need_grad_x else None
    if S == 0 or B == 0:
        out.zero_()
        return grad_x, out
    fn = getattr(L, "whvi_diag_apply_bwd_" + _DTYPE_SUFFIX[x.dtype])
    with _OnDevice(x.device):
        n_slabs = int(L.whvi_diag_apply_bwd_slabs(_DTYPE_CODE[x.dtype], S, B, log2d))      # (sized by x's device's CU count)
        part = torch.empty((S, n_slabs, 2, D), dtype=x.dtype, device=x.device)
        rc = fn(None if grad_x is None else grad_x.data_ptr(), out.data_ptr(), part.data_ptr(), grad_out.data_ptr(),
                x.data_ptr(), s1.data_ptr(), s2.data_ptr(), u.data_ptr(), None if bias is None else bias.data_ptr(), S, B, log2d,
                n_slabs, flags | int(tune), _stream(x))
    _check(rc, "whvi_diag_apply_bwd")
    return grad_x, out


def diag_apply_stacked_supported(dtype: torch.dtype, d: int, n_blocks: int) -> bool:
    """The rule of ``whvi_diag_apply_stacked_supported`` (include/whvi_hip.h), restated so that it needs no library: float32,
    D = 4 .. 4096 a power of two, at least one block, and one sample's diagonals and bias -- 8 J D bytes -- within 64 KiB of LDS."""
    return (dtype == torch.float32 and 4 <= d <= 4096 and (d & (d - 1)) == 0 and n_blocks >= 1 and 8 * n_blocks * d <= 65536)


def diag_apply_stacked(x: torch.Tensor, s1: torch.Tensor, s2: torch.Tensor, u: torch.Tensor, bias: torch.Tensor = None, *,
                       n_samples: int, n_cols: int = None, mean_plus: bool = True, relu_in: bool = False, relu_out: bool = False,
                       out: torch.Tensor = None, tune: int = 0) -> torch.Tensor:
    """One launch: ``out[k, b, j D + i] = x[(k,) b, i] * (wd_j(u[j, 0]) + wd_j(u[j, 1 + k]))_i + bias[j D + i]`` for the first
    ``n_cols`` of the J D columns -- the batched pass of a stacked layer without its matrices; see whvi_diag_apply_stacked_f32
    in include/whvi_hip.h.  ``x``: (S, B, D) or a shared (B, D); ``s1, s2``: (J, D); ``u``: (J, 1 + S, D), or (J, S, D) with
    ``mean_plus=False``; ``bias``: J D elements or None; returns (S, B, n_cols).  ``out``: a (S, B, n_cols) tensor to write,
    rows at any pitch >= n_cols (a column slice of a wider buffer: the columns beyond are left alone)."""
    if x.device.type != "cuda" or x.dtype != torch.float32:
        raise RuntimeError("diag_apply_stacked: float32 CUDA tensors only")
    if s1.dim() != 2 or tuple(s2.shape) != tuple(s1.shape):
        raise RuntimeError("diag_apply_stacked: s1 and s2 must be (n_blocks, D)")
    J, D = s1.shape
    if x.shape[-1] != D or not diag_apply_stacked_supported(x.dtype, D, J):
        raise RuntimeError(f"diag_apply_stacked: D = {x.shape[-1]} with {J} blocks of {D} is outside the supported range")
    S = int(n_samples)
    if x.dim() == 3 and x.shape[0] == S:
        shared, B = False, x.shape[1]
    elif x.dim() == 2:
        shared, B = True, x.shape[0]
    else:
        raise RuntimeError("diag_apply_stacked: x must be (n_samples, batch, D) or (batch, D)")
    U = S + (1 if mean_plus else 0)
    if tuple(u.shape) != (J, U, D):
        raise RuntimeError(f"diag_apply_stacked: u must be ({J}, {U}, {D})")
    _require_f32_on_one_device("diag_apply_stacked", x.device, (s1, s2, u) + (() if bias is None else (bias,)))
    n_cols = J * D if n_cols is None else int(n_cols)
    if not 1 <= n_cols <= J * D:
        raise RuntimeError(f"diag_apply_stacked: n_cols = {n_cols} is outside [1, {J * D}]")
    x, s1, s2, u = _aligned(x), _aligned(s1), _aligned(s2), _aligned(u)
    if bias is not None:
        if bias.numel() != J * D:
            raise RuntimeError("diag_apply_stacked: bias must hold n_blocks * D elements")
        bias = _aligned(bias.reshape(-1))
    if out is None:
        out = torch.empty((S, B, n_cols), dtype=x.dtype, device=x.device)
        ld = n_cols
    else:
        if tuple(out.shape) != (S, B, n_cols) or out.dtype != x.dtype or out.device != x.device:
            raise RuntimeError("diag_apply_stacked: bad out tensor")
        ld = out.stride(1) if B > 1 else (out.stride(0) if S > 1 else n_cols)      # the pitch of the S B rows
        if ld < n_cols or (n_cols > 1 and out.stride(2) != 1) or (B > 1 and S > 1 and out.stride(0) != B * ld):
            raise RuntimeError("diag_apply_stacked: out must be S B rows at one pitch >= n_cols")
    flags = ((DIAG_X_SHARED if shared else 0) | (DIAG_MEAN_PLUS if mean_plus else 0) | (DIAG_RELU_IN if relu_in else 0) |
             (DIAG_RELU_OUT if relu_out else 0))
    with _OnDevice(x.device):
        rc = lib().whvi_diag_apply_stacked_f32(out.data_ptr(), x.data_ptr(), s1.data_ptr(), s2.data_ptr(), u.data_ptr(),
                                               None if bias is None else bias.data_ptr(), S, B, D.bit_length() - 1, J, n_cols,
                                               int(ld), flags | int(tune), _stream(x))
    _check(rc, "whvi_diag_apply_stacked")
    return out


def diag_apply_stacked_bwd_supported(dtype: torch.dtype, d: int, n_blocks: int) -> bool:
    """The rule of ``whvi_diag_apply_stacked_bwd_supported`` (include/whvi_hip.h), restated so that it needs no library: float32,
    D = 4 .. 4096 a power of two, at least one block, and a row of J D <= 8192 columns (eight 16-byte chunks per thread)."""
    return (dtype == torch.float32 and 4 <= d <= 4096 and (d & (d - 1)) == 0 and n_blocks >= 1 and n_blocks * d <= 8192)


def diag_apply_stacked_bwd(grad_out: torch.Tensor, x: torch.Tensor, s1: torch.Tensor, s2: torch.Tensor, u: torch.Tensor, *,
                           n_samples: int, n_cols: int = None, mean_plus: bool = True, need_grad_x: bool = True,
                           bias: torch.Tensor = None, relu_in: bool = False, relu_out: bool = False, tune: int = 0):
    """Backward of ``diag_apply_stacked`` in one call (whvi_diag_apply_stacked_bwd_f32): ``(grad_x (S, B, D) or None, out (4, J,
    U, D))`` with ``out`` as that call documents it -- per block ``diag_apply_bwd``'s slots (0 dL/du, 1 / 2 the per-sample
    shares of dL/ds1 / dL/ds2, 3 of dL/dbias; with ``mean_plus`` row 0 is left for the caller's sum over rows 1 ..), zeros from
    column ``n_cols`` on.  ``grad_out``: (S, B, n_cols), taken at its own pitch when its S B rows have one (a column slice of
    a wider buffer), made contiguous otherwise.  ``x``: the forward's input; ``bias``: the forward's, read only with
    ``relu_out`` (its mask is recomputed)."""
    if x.device.type != "cuda" or x.dtype != torch.float32:
        raise RuntimeError("diag_apply_stacked_bwd: float32 CUDA tensors only")
    if s1.dim() != 2 or tuple(s2.shape) != tuple(s1.shape):
        raise RuntimeError("diag_apply_stacked_bwd: s1 and s2 must be (n_blocks, D)")
    J, D = s1.shape
    if x.shape[-1] != D or not diag_apply_stacked_bwd_supported(x.dtype, D, J):
        raise RuntimeError(f"diag_apply_stacked_bwd: D = {x.shape[-1]} with {J} blocks of {D} is outside the supported range")
    S = int(n_samples)
    if x.dim() == 3 and x.shape[0] == S:
        shared, B = False, x.shape[1]
    elif x.dim() == 2:
        shared, B = True, x.shape[0]
    else:
        raise RuntimeError("diag_apply_stacked_bwd: x must be (n_samples, batch, D) or (batch, D)")
    U = S + (1 if mean_plus else 0)
    if tuple(u.shape) != (J, U, D):
        raise RuntimeError(f"diag_apply_stacked_bwd: u must be ({J}, {U}, {D})")
    _require_f32_on_one_device("diag_apply_stacked_bwd", x.device, (grad_out, s1, s2, u) + (() if bias is None else (bias,)))
    n_cols = J * D if n_cols is None else int(n_cols)
    if not 1 <= n_cols <= J * D:
        raise RuntimeError(f"diag_apply_stacked_bwd: n_cols = {n_cols} is outside [1, {J * D}]")
    if tuple(grad_out.shape) != (S, B, n_cols):
        raise RuntimeError(f"diag_apply_stacked_bwd: grad_out must be ({S}, {B}, {n_cols})")
    x, s1, s2, u = _aligned(x), _aligned(s1), _aligned(s2), _aligned(u)
    if bias is not None:
        if bias.numel() != J * D:
            raise RuntimeError("diag_apply_stacked_bwd: bias must hold n_blocks * D elements")
        bias = _aligned(bias.reshape(-1)) if relu_out else None
    ld = grad_out.stride(1) if B > 1 else (grad_out.stride(0) if S > 1 else n_cols)      # the pitch of the S B rows
    if (ld < n_cols or (n_cols > 1 and grad_out.stride(2) != 1) or (B > 1 and S > 1 and grad_out.stride(0) != B * ld)
            or grad_out.data_ptr() % 4):
        grad_out, ld = grad_out.contiguous(), n_cols
    out = torch.empty((4, J, U, D), dtype=x.dtype, device=x.device)
    grad_x = torch.empty((S, B, D), dtype=x.dtype, device=x.device) if need_grad_x else None
    if S == 0 or B == 0:
        out.zero_()
        return grad_x, out
    L = lib()
    log2d = D.bit_length() - 1
    flags = ((DIAG_X_SHARED if shared else 0) | (DIAG_MEAN_PLUS if mean_plus else 0) | (DIAG_RELU_IN if relu_in else 0) |
             (DIAG_RELU_OUT if relu_out else 0))
    with _OnDevice(x.device):
        n_slabs = int(L.whvi_diag_apply_stacked_bwd_slabs(S, B, log2d, J, n_cols))      # (sized by x's device's CU count)
        part = torch.empty((S, n_slabs, 2, -(-n_cols // 4) * 4), dtype=x.dtype, device=x.device)      # (the written columns only)
        rc = L.whvi_diag_apply_stacked_bwd_f32(None if grad_x is None else grad_x.data_ptr(), out.data_ptr(), part.data_ptr(),
                                               grad_out.data_ptr(), x.data_ptr(), s1.data_ptr(), s2.data_ptr(), u.data_ptr(),
                                               None if bias is None else bias.data_ptr(), S, B, log2d, J, n_cols, int(ld), n_slabs,
                                               flags | int(tune), _stream(x))
    _check(rc, "whvi_diag_apply_stacked_bwd")
    return grad_x, out


APPLY_RELU_IN, APPLY_RELU_OUT = 1, 2


def small_k_apply_supported(x: torch.Tensor, n_out: int) -> bool:
    """Shapes ``whvi_small_k_apply_f32`` covers: a float32 (B, 4) or (B, 8) GPU input, N a multiple of 4 that fits the LDS."""
    k = x.shape[-1]
    if not (x.device.type == "cuda" and x.dtype == torch.float32 and x.dim() == 2 and k in (4, 8) and n_out >= 4 and n_out % 4 == 0):
        return False
    cpr, tpr = n_out // 4, 1
    while tpr < 256 and cpr % (tpr * 2) == 0:
        tpr *= 2
    return cpr // tpr <= 4


def small_k_apply(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor = None, relu_out: bool = False) -> torch.Tensor:
    """One launch: ``out[s] = x @ w[s].T (+ bias)`` for a narrow input shared by all samples -- x (B, K), K in {4, 8};
    w (S, N, K); out (S, B, N); see whvi_small_k_apply_f32 in include/whvi_hip.h."""
    S, N, K = w.shape
    if not small_k_apply_supported(x, N) or w.dtype != torch.float32 or w.device != x.device or x.shape[1] != K:
        raise RuntimeError("small_k_apply: unsupported operands")
    x, w = _aligned(x), _aligned(w)
    if bias is not None:
        bias = _aligned(bias.reshape(-1))
        if bias.numel() != N:
            raise RuntimeError("small_k_apply: bias must hold N elements")
    B = x.shape[0]
    out = torch.empty((S, B, N), dtype=torch.float32, device=x.device)
    with _OnDevice(x.device):
        rc = lib().whvi_small_k_apply_f32(out.data_ptr(), x.data_ptr(), w.data_ptr(), None if bias is None else bias.data_ptr(),
                                          S, B, N, K.bit_length() - 1, APPLY_RELU_OUT if relu_out else 0, _stream(x))
    _check(rc, "whvi_small_k_apply")
    return out


def row_dot_supported(x: torch.Tensor) -> bool:
    d = x.shape[-1]
    return x.device.type == "cuda" and x.dtype == torch.float32 and x.dim() == 3 and 4 <= d <= 4096 and (d & (d - 1)) == 0


def row_dot(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor = None, relu_in: bool = False) -> torch.Tensor:
    """One launch: ``y[s, b] = x[s, b, :] . w[s] (+ bias)`` -- x (S, B, D), w (S, D), y (S, B, 1); see whvi_row_dot_f32."""
    if not row_dot_supported(x) or tuple(w.shape) != (x.shape[0], x.shape[2]) or w.dtype != torch.float32:
        raise RuntimeError("row_dot: unsupported operands")
    x, w = _aligned(x), _aligned(w)
    S, B, D = x.shape
    y = torch.empty((S, B, 1), dtype=torch.float32, device=x.device)
    if bias is not None:
        bias = bias.reshape(-1).contiguous()
    with _OnDevice(x.device):
        rc = lib().whvi_row_dot_f32(y.data_ptr(), x.data_ptr(), w.data_ptr(), None if bias is None else bias.data_ptr(), S, B,
                                    D.bit_length() - 1, APPLY_RELU_IN if relu_in else 0, _stream(x))
    _check(rc, "whvi_row_dot")
    return y


MLP_FIRST_COLUMN, MLP_FIRST_K4, MLP_FIRST_K8 = 1, 4, 8      # whvi_mlp_apply_f32's first-layer kinds (= K; 1 = column)
MLP_ACTS = {"relu": 1, "sigmoid": 2, "tanh": 3}             # whvi_mlp_apply_act_f32's WHVI_MLP_ACT_*


def _mlp_act(act: str) -> int:
    if act not in MLP_ACTS:
        raise RuntimeError(f"mlp_apply: unknown activation {act!r} (one of {', '.join(MLP_ACTS)})")
    return MLP_ACTS[act]


def _mlp_supported(first: int, n_mid: int, d: int, vectors: int) -> bool:
    """First-layer kind 1 / 4 / 8, 1 .. 4 square layers, D = 64 .. 2048 a power of two, and one sample's operands -- 4 D
    (K + 2 + ``vectors`` n_mid) bytes, ``vectors`` D-vectors per square layer -- within 64 KiB of LDS."""
    return (first in (MLP_FIRST_COLUMN, MLP_FIRST_K4, MLP_FIRST_K8) and 1 <= n_mid <= 4 and 64 <= d <= 2048
            and (d & (d - 1)) == 0 and 4 * d * (first + 2 + vectors * n_mid) <= 65536)


def mlp_apply_supported(first: int, n_mid: int, d: int) -> bool:
    """The rule of ``whvi_mlp_apply_supported`` (include/whvi_hip.h), restated so that it needs no library: ``_mlp_supported``
    with 2 vectors per square layer (its diagonal and its bias)."""
    return _mlp_supported(first, n_mid, d, 2)


def mlp_fastfood_apply_supported(first: int, n_mid: int, d: int) -> bool:
    """The rule of ``whvi_mlp_fastfood_apply_supported`` (include/whvi_hip.h) without the library: ``_mlp_supported`` with 4
    vectors per square layer (s1, s2, g_k and the bias)."""
    return _mlp_supported(first, n_mid, d, 4)


def mlp_apply_bwd_supported(first: int, n_mid: int, d: int) -> bool:
    """The rule of ``whvi_mlp_apply_bwd_supported`` (include/whvi_hip.h) without the library: ``mlp_apply_supported`` with at
    most 2 square layers and D <= 1024."""
    return mlp_apply_supported(first, n_mid, d) and n_mid <= 2 and d <= 1024


def mlp_fastfood_apply_bwd_supported(first: int, n_mid: int, d: int) -> bool:
    """The rule of ``whvi_mlp_fastfood_apply_bwd_supported`` (include/whvi_hip.h) without the library:
    ``mlp_fastfood_apply_supported`` with at most 2 square layers and D <= 1024."""
    return mlp_fastfood_apply_supported(first, n_mid, d) and n_mid <= 2 and d <= 1024


def _ptr(t):
    return None if t is None else t.data_ptr()


def _mlp_operands(what, supported, act, x, w_in, b_in, s1, s2, mid, mid_rows, b_mid, mid_bias, w_out, b_out=None, g=None):
    """The operands of the four network launches, checked once: ``what`` names the caller in every refusal, ``supported`` is
    its range rule, ``mid`` the per-layer tensor, expected as ``(n_mid, mid_rows, D)`` with ``mid_rows`` counted beyond S (1 for
    ``u`` and its mean row, 0 for ``g``).  ``g`` = dL/dy (S, B) is the backward's extra operand; a backward has no ``b_out``.
    Returns ``(code, first, n_mid, S, B, D, args, keep)``: the activation code, the sizes, the C entry points' shared argument
    block ([g,] x .. w_out[, b_out], S, B, log2d) and the contiguous, aligned tensors behind its pointers, which the caller
    holds until it has launched."""
    code = _mlp_act(act)
    S, D = w_out.shape
    n_mid = s1.shape[0]
    first = MLP_FIRST_COLUMN if w_in.dim() == 2 else w_in.shape[2]
    if not supported(first, n_mid, D):
        raise RuntimeError(f"{what}: unsupported network (first layer {first}, {n_mid} square layers, D = {D})")
    ops = (x, w_in, s1, s2, mid, w_out) + tuple(t for t in (g, b_in, b_mid, b_out) if t is not None)
    _require_f32_on_one_device(what, x.device, ops)
    B = x.shape[0]
    if ((g is not None and tuple(g.shape) != (S, B)) or tuple(x.shape) != (B, first) or tuple(w_in.shape[:2]) != (S, D)
            or tuple(s1.shape) != (n_mid, D) or tuple(s2.shape) != (n_mid, D) or tuple(mid.shape) != (n_mid, S + mid_rows, D)
            or (b_mid is not None and b_mid.numel() != n_mid * D) or (b_in is not None and b_in.numel() != D)
            or (b_out is not None and b_out.numel() != 1)):
        raise RuntimeError(f"{what}: operand shapes do not match")
    if g is not None:
        g = _aligned(g)
    x, w_in, s1, s2, mid, w_out = (_aligned(t) for t in (x, w_in, s1, s2, mid, w_out))
    b_in, b_mid, b_out = (None if t is None else _aligned(t.reshape(-1)) for t in (b_in, b_mid, b_out))
    args = (x.data_ptr(), first, w_in.data_ptr(), _ptr(b_in), n_mid, s1.data_ptr(), s2.data_ptr(), mid.data_ptr(), _ptr(b_mid),
            int(mid_bias), w_out.data_ptr())
    args = args + (_ptr(b_out),) if g is None else (g.data_ptr(),) + args
    return code, first, n_mid, S, B, D, args + (S, B, D.bit_length() - 1), (g, x, w_in, s1, s2, mid, w_out, b_in, b_mid, b_out)


def mlp_apply(x: torch.Tensor, w_in: torch.Tensor, b_in, s1: torch.Tensor, s2: torch.Tensor, u: torch.Tensor, b_mid,
              w_out: torch.Tensor, b_out, *, mid_bias: int = 0, relu: int = 0, act: str = "relu") -> torch.Tensor:
    """One launch: the predictive pass of a WHVI regression network for all MC samples -- y (S, B); see
    whvi_mlp_apply_f32 in include/whvi_hip.h.  x (B, K) with w_in (S, D, K), K = 4 / 8, or x (B, 1) with w_in (S, D);
    s1, s2 (n_mid, D); u (n_mid, 1 + S, D); b_mid (n_mid, D) or None; w_out (S, D); b_in (D elements) / b_out (1) or None.
    ``mid_bias`` bit m: square layer m has a bias; ``relu``: the boundaries that carry the activation ``act`` -- bit 0 behind
    the first layer, bit 1 + m behind square layer m.  ``act``: "relu" (whvi_mlp_apply_f32), "sigmoid" or "tanh"
    (whvi_mlp_apply_act_f32)."""
    code, _, _, S, B, _, args, keep = _mlp_operands("mlp_apply", mlp_apply_supported, act, x, w_in, b_in, s1, s2, u, 1, b_mid,
                                                    mid_bias, w_out, b_out)
    y = torch.empty((S, B), dtype=torch.float32, device=x.device)
    with _OnDevice(x.device):
        if act == "relu":
            rc = lib().whvi_mlp_apply_f32(y.data_ptr(), *args, int(relu), _stream(x))
        else:
            rc = lib().whvi_mlp_apply_act_f32(y.data_ptr(), *args, code, int(relu), _stream(x))
    _check(rc, "whvi_mlp_apply")
    return y


def mlp_fastfood_apply(x: torch.Tensor, w_in: torch.Tensor, b_in, s1: torch.Tensor, s2: torch.Tensor, g: torch.Tensor, b_mid,
                       w_out: torch.Tensor, b_out, *, mid_bias: int = 0, act_bits: int = 0, act: str = "relu") -> torch.Tensor:
    """One launch: the predictive pass of a WHVI regression network with fastfood square layers for all MC samples -- y (S, B);
    see whvi_mlp_fastfood_apply_f32 in include/whvi_hip.h.  x, w_in, b_in, w_out, b_out, ``act`` and ``act_bits`` as
    ``mlp_apply``; s1, s2 (n_mid, D); g (n_mid, S, D), every sample's g_k; b_mid (n_mid, D) or None (``mid_bias`` bit m:
    square layer m has a bias)."""
    code, _, _, S, B, _, args, keep = _mlp_operands("mlp_fastfood_apply", mlp_fastfood_apply_supported, act, x, w_in, b_in, s1, s2,
                                                    g, 0, b_mid, mid_bias, w_out, b_out)
    y = torch.empty((S, B), dtype=torch.float32, device=x.device)
    with _OnDevice(x.device):
        rc = lib().whvi_mlp_fastfood_apply_f32(y.data_ptr(), *args, code, int(act_bits), _stream(x))
    _check(rc, "whvi_mlp_fastfood_apply")
    return y


def mlp_apply_bwd(g: torch.Tensor, x: torch.Tensor, w_in: torch.Tensor, b_in, s1: torch.Tensor, s2: torch.Tensor,
                  u: torch.Tensor, b_mid, w_out: torch.Tensor, *, mid_bias: int = 0, relu: int = 0, need_grad_x: bool = False,
                  act: str = "relu"):
    """Backward of ``mlp_apply`` in one call (whvi_mlp_apply_bwd_f32, or whvi_mlp_apply_act_bwd_f32 for ``act`` "sigmoid" /
    "tanh"): ``(grad_w_in, grad_w_mid (n_mid, S, D), grad_w_out (S, D), grad_b ((1 + n_mid) D + 1: b_in, b_mid rows, b_out),
    grad_x (S, B, K) or None)`` from ``g`` = dL/dy (S, B) and the forward's operands (same shapes and ``relu`` / ``act`` as
    ``mlp_apply``)."""
    code, first, n_mid, S, B, D, args, keep = _mlp_operands("mlp_apply_bwd", mlp_apply_bwd_supported, act, x, w_in, b_in, s1, s2,
                                                            u, 1, b_mid, mid_bias, w_out, g=g)
    dev = x.device
    grad_w_in = torch.empty(tuple(w_in.shape), dtype=torch.float32, device=dev)
    grad_w_mid = torch.empty((n_mid, S, D), dtype=torch.float32, device=dev)
    grad_w_out = torch.empty((S, D), dtype=torch.float32, device=dev)
    grad_b = torch.empty(((1 + n_mid) * D + 1,), dtype=torch.float32, device=dev)
    grad_x = torch.empty((S, B, first), dtype=torch.float32, device=dev) if need_grad_x else None
    L = lib()
    with _OnDevice(dev):
        n = int(L.whvi_mlp_apply_bwd_workspace(S, B, first, n_mid, D.bit_length() - 1))
        work = torch.empty((max(n, 1),), dtype=torch.float32, device=dev)
        outs = (grad_w_in.data_ptr(), grad_w_mid.data_ptr(), grad_w_out.data_ptr(), grad_b.data_ptr(), _ptr(grad_x),
                work.data_ptr(), n)
        if act == "relu":
            rc = L.whvi_mlp_apply_bwd_f32(*outs, *args, int(relu), _stream(x))
        else:
            rc = L.whvi_mlp_apply_act_bwd_f32(*outs, *args, code, int(relu), _stream(x))
    _check(rc, "whvi_mlp_apply_bwd")
    return grad_w_in, grad_w_mid, grad_w_out, grad_b, grad_x


def mlp_fastfood_apply_bwd(g: torch.Tensor, x: torch.Tensor, w_in: torch.Tensor, b_in, s1: torch.Tensor, s2: torch.Tensor,
                           gk: torch.Tensor, b_mid, w_out: torch.Tensor, *, mid_bias: int = 0, act_bits: int = 0,
                           need_grad_x: bool = False, act: str = "relu"):
    """Backward of ``mlp_fastfood_apply`` in one call (whvi_mlp_fastfood_apply_bwd_f32): ``(grad_w_in, grad_s1 (n_mid, D),
    grad_s2 (n_mid, D), grad_g (n_mid, S, D), grad_w_out (S, D), grad_b ((1 + n_mid) D + 1: b_in, b_mid rows, b_out),
    grad_x (S, B, K) or None)`` from ``g`` = dL/dy (S, B) and the forward's operands (``gk`` is its ``g``; same shapes,
    ``act_bits`` and ``act`` as ``mlp_fastfood_apply``)."""
    code, first, n_mid, S, B, D, args, keep = _mlp_operands("mlp_fastfood_apply_bwd", mlp_fastfood_apply_bwd_supported, act, x,
                                                            w_in, b_in, s1, s2, gk, 0, b_mid, mid_bias, w_out, g=g)
    dev = x.device
    grad_w_in = torch.empty(tuple(w_in.shape), dtype=torch.float32, device=dev)
    grad_s1 = torch.empty((n_mid, D), dtype=torch.float32, device=dev)
    grad_s2 = torch.empty((n_mid, D), dtype=torch.float32, device=dev)
    grad_g = torch.empty((n_mid, S, D), dtype=torch.float32, device=dev)
    grad_w_out = torch.empty((S, D), dtype=torch.float32, device=dev)
    grad_b = torch.empty(((1 + n_mid) * D + 1,), dtype=torch.float32, device=dev)
    grad_x = torch.empty((S, B, first), dtype=torch.float32, device=dev) if need_grad_x else None
    L = lib()
    with _OnDevice(dev):
        n = int(L.whvi_mlp_fastfood_apply_bwd_workspace(S, B, first, n_mid, D.bit_length() - 1))
        work = torch.empty((max(n, 1),), dtype=torch.float32, device=dev)
        rc = L.whvi_mlp_fastfood_apply_bwd_f32(grad_w_in.data_ptr(), grad_s1.data_ptr(), grad_s2.data_ptr(), grad_g.data_ptr(),
                                               grad_w_out.data_ptr(), grad_b.data_ptr(), _ptr(grad_x), work.data_ptr(), n,
                                               *args, code, int(act_bits), _stream(x))
    _check(rc, "whvi_mlp_fastfood_apply_bwd")
    return grad_w_in, grad_s1, grad_s2, grad_g, grad_w_out, grad_b, grad_x


def reparam_kl_bwd(grad_u, grad_kl, g_mu, g_rho, eps, sigma, lambda_: float):
    """One launch: (grad_mu, grad_rho), each (J, D); see whvi_reparam_kl_bwd_f32 in include/whvi_hip.h.
    ``grad_u`` (J, 1+S, D) and ``grad_kl`` (J,) may be None (= zero)."""
    J, D = g_mu.shape
    S = eps.shape[1]
    grad_u = None if grad_u is None else grad_u.contiguous()
    grad_kl = None if grad_kl is None else grad_kl.contiguous()
    out = torch.empty((2, J, D), dtype=torch.float32, device=g_mu.device)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with _OnDevice(g_mu.device):
        rc = lib().whvi_reparam_kl_bwd_f32(out[0].data_ptr(), out[1].data_ptr(), ptr(grad_u), ptr(grad_kl),
                                           g_mu.data_ptr(), g_rho.data_ptr(), eps.data_ptr() if S > 0 else None,
                                           sigma.data_ptr(), J, S, D, float(lambda_), _stream(g_mu))
    _check(rc, "whvi_reparam_kl_bwd")
    return out[0], out[1]


def _mnll_dims(y: torch.Tensor, y_hat: torch.Tensor):
    """Three (size, y_hat stride, y stride) triples, dimensions ordered by decreasing y_hat stride (memory order)."""
    order = sorted(range(3), key=lambda k: -y_hat.stride(k))
    arr = ctypes.c_int64 * 3
    return (arr(*[y_hat.size(k) for k in order]), arr(*[y_hat.stride(k) for k in order]),
            arr(*[y.stride(k) for k in order]))


def gauss_mnll(y: torch.Tensor, y_hat: torch.Tensor, sigma: torch.Tensor, scale: float):
    """Per-block partial sums (blocks, 2) of whvi_gauss_mnll_f32: ``y_hat`` (m, n_out, n_mc) with any strides,
    ``y`` an expanded view of the same shape, ``sigma`` a device scalar."""
    L = lib()
    part = torch.empty((L.whvi_gauss_mnll_blocks(y_hat.numel()), 2), dtype=torch.float32, device=y_hat.device)
    size, hs, ys = _mnll_dims(y, y_hat)
    with _OnDevice(y_hat.device):
        rc = L.whvi_gauss_mnll_f32(part.data_ptr(), y.data_ptr(), y_hat.data_ptr(), sigma.data_ptr(), size, hs, ys,
                                   float(scale), _stream(y_hat))
    _check(rc, "whvi_gauss_mnll")
    return part


def decay_lr_step(t: torch.Tensor, lr: torch.Tensor, base_lr: float, lambda0: float, gamma: float, p: float,
                  advance: bool = True) -> None:
    """whvi_decay_lr_step: ``t`` (0-d float64) += 1 when ``advance``; ``lr`` (0-d float32) <- base_lr * lambda0 *
    (1 + gamma t)^-p.  One single-thread launch on the current stream (capture-safe)."""
    if t.dtype != torch.float64 or lr.dtype != torch.float32 or t.numel() != 1 or lr.numel() != 1 or t.device != lr.device \
            or t.device.type != "cuda":
        raise RuntimeError("decay_lr_step: t must be a float64 and lr a float32 device scalar on the same GPU")
    with _OnDevice(t.device):
        rc = lib().whvi_decay_lr_step(t.data_ptr(), lr.data_ptr(), float(base_lr), float(lambda0), float(gamma), float(p),
                                      1 if advance else 0, _stream(t))
    _check(rc, "whvi_decay_lr_step")


def gauss_mnll_bwd(grad_out, part, y, y_hat, sigma, scale: float):
    """(grad_yhat with y_hat's strides, grad_sigma scalar) of whvi_gauss_mnll_bwd_f32."""
    grad_yhat = torch.empty_strided(y_hat.size(), y_hat.stride(), dtype=torch.float32, device=y_hat.device)
    grad_sigma = torch.empty((), dtype=torch.float32, device=y_hat.device)
    size, hs, ys = _mnll_dims(y, y_hat)
    with _OnDevice(y_hat.device):
        rc = lib().whvi_gauss_mnll_bwd_f32(grad_yhat.data_ptr(), grad_sigma.data_ptr(), grad_out.data_ptr(),
                                           part.data_ptr(), y.data_ptr(), y_hat.data_ptr(), sigma.data_ptr(), size, hs,
                                           ys, float(scale), _stream(y_hat))
    _check(rc, "whvi_gauss_mnll_bwd")
    return grad_yhat, grad_sigma
