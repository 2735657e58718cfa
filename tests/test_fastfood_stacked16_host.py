"""The rectangular fastfood layer on 16-bit activations (whvi_fused_shs_stacked_f16 / _bf16, ``FastfoodStackedFunction`` with
``keep_half``) as far as it can be checked without a GPU: the ABI declares and exports the three symbols, the support rule and
its Python mirror, every refusal (ctypes with fake aligned pointers: the checks happen before any device call; extents for
2-byte activations and 4-byte vectors), what the shipped library contains -- a fused_stacked16_kernel<T, L, fused_bwd_k(L, 8),
NT> for both storage types and every L in 6 .. 11, none with scratch -- and that host tensors keep the composed route."""
import ctypes
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("whvi_fused_shs_stacked16_supported", "whvi_fused_shs_stacked_f16", "whvi_fused_shs_stacked_bf16")
SRC_SHARED = 4


def test_header_declares_and_library_exports_the_three_symbols():
    from whvi_amd import _hip
    raw = open(os.path.join(ROOT, "include", "whvi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(whvi_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert "#define WHVI_HIP_ABI_VERSION 1" in raw
    assert _hip.lib().whvi_hip_abi_version() == 1


def test_support_rule_and_its_mirror():
    from whvi_amd import _hip
    L = _hip.lib()
    for log2d in range(0, 16):
        for J in (-1, 0, 1, 2, 3, 5, 6, 21, 22, 42, 43, 85, 86, 1 << 40):
            rule = 6 <= log2d <= 11 and J >= 1 and 12 * (1 << log2d) * J <= 65536
            assert L.whvi_fused_shs_stacked16_supported(log2d, J) == int(rule), (log2d, J)
            for dtype in (torch.float16, torch.bfloat16):
                assert _hip.fused_shs_stacked16_supported(dtype, 1 << log2d, J) == rule, (dtype, log2d, J)
            for dtype in (torch.float32, torch.float64):
                assert not _hip.fused_shs_stacked16_supported(dtype, 1 << log2d, J), (dtype, log2d, J)
    assert _hip.fused_shs_stacked16_supported(torch.float16, 256, 2) and _hip.fused_shs_stacked16_supported(torch.bfloat16, 256, 2)
    assert not _hip.fused_shs_stacked16_supported(torch.float16, 100, 2)
    # the float32 launch's predicate keeps refusing 16-bit storage
    assert not _hip.fused_shs_stacked_supported(torch.float16, 256, 2)
    assert not _hip.fused_shs_stacked_supported(torch.bfloat16, 256, 2)


def test_refusals_before_any_device_call():
    from whvi_amd import _hip
    for entry in ENTRIES[1:]:
        fn = getattr(_hip.lib(), entry)
        buf = (ctypes.c_char * (1 << 20))()
        p = (ctypes.addressof(buf) + 15) & ~15
        K = 65536                 # J = 2, S = 2, stride = 2, D = 512: dst 8 KiB, src 4 KiB (2 shared), a / c 4 KiB, b 8 KiB
        dst, src, a, b, c = (p + i * K for i in range(5))

        def call(dst=dst, src=src, a=a, b=b, c=c, J=2, S=2, stride=2, log2d=9, flags=0):
            return fn(dst, src, a, b, c, J, S, stride, log2d, flags, None)

        err = _hip.last_error
        assert call(flags=1) == -1 and "unknown fused flags" in err()
        assert call(flags=8) == -1 and "unknown fused flags" in err()
        assert call(flags=SRC_SHARED | 16) == -1 and "unknown fused flags" in err()
        for name in ("dst", "src", "a", "b", "c"):
            assert call(**{name: None}) == -1 and "null" in err(), name
        assert call(J=-1) == -1 and "negative" in err()
        assert call(S=-1) == -1 and call(stride=-1) == -1
        for log2d in (-1, 0, 5, 12, 13):
            assert call(log2d=log2d) == -2 and "supported range" in err(), log2d
        assert call(J=0) == -2
        assert call(J=11) == -2 and "LDS" in err()                          # 12 * 512 * 11 > 65536
        assert call(J=10, S=0) == 0
        assert call(log2d=11, J=3) == -2 and call(log2d=6, J=86) == -2
        assert call(S=1 << 20, stride=1 << 12) == -2 and "32 bits" in err()
        for name, ptr in (("dst", dst), ("src", src), ("a", a), ("b", b), ("c", c)):
            assert call(**{name: ptr + 4}) == -3 and "aligned" in err(), name
        # dst (8 KiB of 2-byte elements) over each input: src 4 KiB, a and c 4 KiB, b 8 KiB
        assert call(dst=src) == -5 and "overlap" in err()
        assert call(dst=src + 4096 - 16) == -5 and call(dst=src - 8192 + 16) == -5
        assert call(dst=a + 4080) == -5 and call(dst=b + 8176) == -5 and call(dst=c - 16) == -5
        assert call(dst=src + 2048 - 16, flags=SRC_SHARED) == -5           # (a shared source is sample_stride rows: 2 KiB)
        # nothing to do: accepted without touching a pointer or a device
        assert call(S=0) == 0 and err() == ""
        assert call(stride=0) == 0 and err() == ""
        assert fn(None, None, None, None, None, 2, 0, 7, 9, 0, None) == 0
        assert fn(None, None, None, None, None, 1, 3, 0, 11, SRC_SHARED, None) == 0


def _shipped():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    return shipped_isa.ShippedLibrary()


def test_shipped_library_has_every_instantiation():
    with _shipped() as lib:
        kernels = lib.kernels
    mine = {n: k for n, k in kernels.items() if "fused_stacked16_kernel<" in n}
    k_of = {6: 2, 7: 2, 8: 2, 9: 2, 10: 2, 11: 4}                           # fused_bwd_k(L, 8)
    want = {f"whvi::fused_stacked16_kernel<{t}, {L}, {k_of[L]}, {nt}>" for t in ("__half", "__hip_bfloat16") for L in range(6, 12)
            for nt in ("true", "false")}
    assert set(mine) == want
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgprs"] + k["agprs"] <= 256, (name, k)


def test_host_tensors_keep_the_composed_route():
    """``keep_half`` applies to CUDA tensors only: on the host a float16 input is promoted by the first multiply, block by block,
    exactly as before, and no launch is named."""
    from whvi_amd import _hip
    from whvi_amd.fastfood import FastfoodStackedFunction, _pipeline
    J, S, B, D = 3, 2, 5, 64
    g = torch.Generator().manual_seed(16)
    a, c = (torch.randn(J, D, generator=g) for _ in range(2))
    b = torch.randn(J, S, D, generator=g)
    before = _hip.last_kernel()
    for shared in (False, True):
        x = torch.randn(B if shared else S * B, D, generator=g).half()
        want = torch.cat([_pipeline(x, a[j], b[j], c[j], S, B, shared, False) for j in range(J)], dim=1)
        for keep_half in (True, False):
            got = FastfoodStackedFunction.apply(x, a, b, c, S, B, shared, keep_half, False)
            assert got.dtype == torch.float32 and got.shape == (S * B, J * D)
            assert torch.equal(got, want)
        xf = x.float().repeat(S, 1) if shared else x.float()
        rows = torch.arange(S * B) // B % S
        for j in range(J):
            import fwht_cpp
            ref = a[j] * fwht_cpp.forward(b[j][rows] * fwht_cpp.forward(c[j] * xf))
            assert torch.equal(want[:, j * D:(j + 1) * D], ref)
    assert _hip.last_kernel() == before and "fused_stacked16_kernel" not in before
