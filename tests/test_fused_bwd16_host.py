"""The one-launch backward of the fused pipeline on 16-bit activation streams (whvi_fused_shs_bwd_f16 / _bf16) as far as it can
be checked without a GPU: the ABI declares and exports both entries, ``_hip.fused_shs_bwd16_supported``, the argument checks
(ctypes with fake aligned pointers: every check happens before any device call; the extents of grad_x, grad_y and x are counted
in 2-byte elements), what the shipped library contains -- a fused_shs_bwd_kernel<__half | __hip_bfloat16, L, K, NT> for every L
in 6 .. 12 in both NT forms, none with scratch, beside the unchanged float32 backward symbols and the pinned
fused_shs_kernel<float|double, ...> set -- and that ``keep_half`` with ``fused_backward`` changes nothing on host tensors."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("whvi_fused_shs_bwd_f16", "whvi_fused_shs_bwd_bf16")
TYPES = ("__half", "__hip_bfloat16")
SRC_SHARED = 4
# chunks per lane of the tile: the float32 kernel's rows in 8-element chunks
K16 = {6: 2, 7: 2, 8: 2, 9: 2, 10: 2, 11: 4, 12: 8}
K32 = {6: 4, 7: 4, 8: 4, 9: 4, 10: 4, 11: 8, 12: 16}


def test_header_declares_and_library_exports_both_entries():
    from whvi_amd import _hip
    raw = open(os.path.join(ROOT, "include", "whvi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(whvi_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert hasattr(_hip.lib(), name) and getattr(_hip.lib(), name).argtypes is not None, name
    assert "#define WHVI_HIP_ABI_VERSION 1" in raw
    assert _hip.lib().whvi_hip_abi_version() == 1


def test_supported_query_is_exact():
    from whvi_amd import _hip
    for d in (32, 64, 4096, 8192):
        for dtype in (torch.float16, torch.bfloat16):
            assert _hip.fused_shs_bwd16_supported(dtype, d) == (64 <= d <= 4096), (dtype, d)
            assert not _hip.fused_shs_bwd_supported(dtype, d)           # (the float32 query stays float32-only)
        for dtype in (torch.float32, torch.float64, torch.int32):
            assert not _hip.fused_shs_bwd16_supported(dtype, d), (dtype, d)
    for d in (0, -64, 96, 1000):
        assert not _hip.fused_shs_bwd16_supported(torch.float16, d)
    for log2d in range(6, 13):
        assert _hip.fused_shs_bwd16_supported(torch.bfloat16, 1 << log2d)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_checks_before_any_device_call(entry):
    from whvi_amd import _hip
    bwd = getattr(_hip.lib(), entry)
    buf = (ctypes.c_char * (1 << 20))()
    p = (ctypes.addressof(buf) + 15) & ~15
    K = 32768                                       # S = 2, stride = 2, D = 512: an activation is 4 KiB, b 4 KiB, a / c 2 KiB
    gx, ga, gb, gc, work, gy, x, a, b, c = (p + i * K for i in range(10))

    def call(gx=gx, ga=ga, gb=gb, gc=gc, work=work, gy=gy, x=x, a=a, b=b, c=c, S=2, stride=2, log2d=9, flags=0):
        return bwd(gx, ga, gb, gc, work, gy, x, a, b, c, S, stride, log2d, flags, None)

    def err():
        return _hip.last_error()

    for name in ("ga", "gb", "gc", "work", "gy", "x", "a", "b", "c"):
        assert call(**{name: None}) == -1 and "null" in err(), name
    assert call(flags=1) == -1 and "unknown fused flags" in err()
    assert call(flags=8) == -1 and "unknown fused flags" in err()
    assert call(flags=SRC_SHARED | 16) == -1 and "unknown fused flags" in err()
    assert call(S=-1) == -1 and call(stride=-1) == -1
    for log2d in (-1, 0, 5, 13, 14):
        assert call(log2d=log2d) == -2 and "supported range" in err(), log2d
    assert call(S=1 << 20, stride=1 << 12) == -2 and "32 bits" in err()
    assert call(S=(1 << 22) - 2, stride=1, log2d=9) == -2 and "32 bits" in err()        # (S + 2) D reaches 2^31
    for name, ptr in (("gx", gx), ("ga", ga), ("gb", gb), ("gc", gc), ("work", work), ("gy", gy), ("x", x), ("a", a), ("b", b),
                      ("c", c)):
        assert call(**{name: ptr + 4}) == -3 and "aligned" in err(), name
        assert call(**{name: ptr + 2}) == -3 and "aligned" in err(), name
    # grad_x (4 KiB: 2-byte elements) over each input, from either side down to the last 16 bytes
    assert call(gx=gy) == -5 and "overlap" in err()
    assert call(gx=gy + 4096 - 16) == -5 and call(gx=gy - 4096 + 16) == -5
    assert call(gx=x + 2048) == -5 and call(gx=x + 4080) == -5 and call(gx=x - 4080) == -5
    assert call(gx=a - 16) == -5 and call(gx=a + 2032) == -5 and call(gx=b + 4080) == -5 and call(gx=c) == -5
    assert call(gx=x + 2032, flags=SRC_SHARED) == -5                      # (a shared x is sample_stride rows: 2 KiB)
    # the float32 outputs keep 4-byte extents: grad_a / grad_c 2 KiB, grad_b 4 KiB
    assert call(ga=a) == -5 and call(ga=gy - 2032) == -5 and call(gb=b + 16) == -5 and call(gb=gy - 4080) == -5
    assert call(gc=gy) == -5 and call(gc=gy + 4080) == -5 and call(work=x) == -5 and call(work=x + 4080) == -5
    # nothing to do: accepted without touching a pointer or a device
    assert call(S=0) == 0 and err() == ""
    assert call(stride=0) == 0 and err() == ""
    assert bwd(None, None, None, None, None, None, None, None, None, None, 0, 7, 9, 0, None) == 0
    assert bwd(None, None, None, None, None, None, None, None, None, None, 3, 0, 12, SRC_SHARED, None) == 0


def _shipped():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    return shipped_isa.ShippedLibrary()


def test_shipped_library_has_every_16_bit_instantiation_without_scratch_and_keeps_the_other_symbols():
    with _shipped() as lib:
        kernels = lib.kernels
    for t in TYPES:
        for log2d in range(6, 13):
            want = {f"whvi::fused_shs_bwd_kernel<{t}, {log2d}, {K16[log2d]}, {nt}>" for nt in ("true", "false")}
            mine = {n: k for n, k in kernels.items() if n.startswith(f"whvi::fused_shs_bwd_kernel<{t}, {log2d}, ")}
            assert set(mine) == want, (t, log2d, sorted(mine))
            for name, k in mine.items():
                assert k["scratch"] == 0, (name, k)
                assert k["vgprs"] + k["agprs"] <= 512, (name, k)
                if log2d <= 11:
                    assert k["vgprs"] + k["agprs"] <= 256, (name, k)    # at least two waves per SIMD below the one-row tile of 4096
                assert k["lds"] == 0, (name, k)                         # (dynamic: 12 D bytes given at the launch)
    # the float32 backward: the same fourteen symbols and the finishing kernel, nothing else in the family
    family = sorted(n for n in kernels if n.startswith("whvi::fused_shs_bwd_kernel<"))
    f32 = sorted(f"whvi::fused_shs_bwd_kernel<float, {log2d}, {K32[log2d]}, {nt}>" for log2d in range(6, 13)
                 for nt in ("true", "false"))
    assert [n for n in family if "<float, " in n] == f32
    assert len(family) == 3 * 14, family
    assert any(n.startswith("whvi::fused_shs_bwd_finish_kernel") for n in kernels)
    golden = [g for g in open(os.path.join(ROOT, "tests", "golden", "fused_shs_kernel_symbols_f32_f64.txt")).read().split("\n")
              if g.strip()]
    now = sorted(n for n in kernels if re.match(r"whvi::fused_shs_kernel<(float|double), ", n))
    assert now == sorted(golden), "the float / double instantiations of fused_shs_kernel changed"


def test_both_flags_are_ignored_on_host_tensors():
    from whvi_amd.fastfood import FastfoodFunction, WHVIFastfoodMatrix
    D, S, B = 64, 3, 5
    for shared in (False, True):
        grads = []
        for flags in ((False, False), (True, True)):
            x = torch.randn(B if shared else S * B, D, generator=torch.Generator().manual_seed(1)).requires_grad_()
            a, b, c = (torch.randn(n, generator=torch.Generator().manual_seed(2 + i)).requires_grad_()
                       for i, n in enumerate((D, S * D, D)))
            y = FastfoodFunction.apply(x, a, b.view(S, D), c, S, B, shared, *flags)
            w = torch.randn(y.shape, generator=torch.Generator().manual_seed(9))
            (y * w).sum().backward()
            grads.append((y.detach(), x.grad, a.grad, b.grad, c.grad))
        for u, v in zip(*grads):
            assert u.dtype == torch.float32 and torch.equal(u, v)
    assert WHVIFastfoodMatrix.fused_backward is False and WHVIFastfoodMatrix.keep_half is False
    outs = []
    for flag in (False, True):
        torch.manual_seed(3)
        layer = WHVIFastfoodMatrix(D)
        layer.fused_backward = layer.keep_half = flag
        x = torch.randn(S, B, D, generator=torch.Generator().manual_seed(4)).requires_grad_()
        loss = layer.forward_mc(x, S).square().sum()
        loss.backward()
        outs.append([loss.detach(), x.grad] + [p.grad for p in layer.parameters()])
    for u, v in zip(*outs):
        assert torch.equal(u, v)
