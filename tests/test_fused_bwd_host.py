"""The one-launch backward of the fused pipeline (whvi_fused_shs_bwd_f32) as far as it can be checked without a GPU: the ABI
declares and exports the three symbols, the argument checks (ctypes with fake aligned pointers: every check happens before
any device call), the support and workspace queries, what the shipped library contains -- a fused_shs_bwd_kernel<float, L, ...>
for every L in 6 .. 12, none with scratch, and the unchanged set of fused_shs_kernel<float|double, ...> symbols -- and that
``fused_backward`` is ignored on host tensors."""
import ctypes
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("whvi_fused_shs_bwd_supported", "whvi_fused_shs_bwd_workspace", "whvi_fused_shs_bwd_f32")
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


def test_supported_exactly_6_to_12_and_workspace_query():
    from whvi_amd import _hip
    L = _hip.lib()
    for log2d in range(-2, 20):
        assert L.whvi_fused_shs_bwd_supported(log2d) == (1 if 6 <= log2d <= 12 else 0), log2d
    for d in (32, 64, 4096, 8192):
        assert _hip.fused_shs_bwd_supported(torch.float32, d) == (64 <= d <= 4096)
        assert not _hip.fused_shs_bwd_supported(torch.float64, d)
        assert not _hip.fused_shs_bwd_supported(torch.float16, d)
    for log2d in range(6, 13):
        for S, stride in ((1, 1), (3, 5), (2, 777), (4, 64), (64, 8192), (1, 1 << 20)):
            n = L.whvi_fused_shs_bwd_workspace(S, stride, log2d)
            assert n > 0 and n % 16 == 0, (S, stride, log2d, n)
            assert n % (12 << log2d) == 0 and (n // (12 << log2d)) % S == 0          # whole slots, the same count per sample
            assert n == L.whvi_fused_shs_bwd_workspace(S, stride, log2d)            # a function of the arguments alone
        assert L.whvi_fused_shs_bwd_workspace(0, 5, log2d) == 0 and L.whvi_fused_shs_bwd_workspace(5, 0, log2d) == 0
    assert L.whvi_fused_shs_bwd_workspace(4, 64, 13) == -2
    assert L.whvi_fused_shs_bwd_workspace(4, 64, 5) == -2
    assert L.whvi_fused_shs_bwd_workspace(-1, 64, 9) == -1
    # one row, one sample: one block; the largest launches stay within 24 MiB
    assert L.whvi_fused_shs_bwd_workspace(1, 1, 9) == 12 << 9
    assert max(L.whvi_fused_shs_bwd_workspace(64, 8192, k) for k in range(6, 13)) <= 24 << 20


def test_argument_checks_before_any_device_call():
    from whvi_amd import _hip
    bwd = _hip.lib().whvi_fused_shs_bwd_f32
    buf = (ctypes.c_char * (1 << 20))()
    p = (ctypes.addressof(buf) + 15) & ~15
    K = 32768                                       # S = 2, stride = 2, D = 512: an activation is 8 KiB, b 4 KiB, a / c 2 KiB
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
    for name, ptr in (("gx", gx), ("ga", ga), ("gb", gb), ("gc", gc), ("work", work), ("gy", gy), ("x", x), ("a", a), ("b", b),
                      ("c", c)):
        assert call(**{name: ptr + 4}) == -3 and "aligned" in err(), name
    # grad_x (8 KiB) over each input
    assert call(gx=gy) == -5 and "overlap" in err()
    assert call(gx=gy + 8192 - 16) == -5 and call(gx=gy - 8192 + 16) == -5
    assert call(gx=x + 4096) == -5 and call(gx=a - 16) == -5 and call(gx=b + 4080) == -5 and call(gx=c) == -5
    assert call(gx=x + 4080, flags=SRC_SHARED) == -5                      # (a shared x is sample_stride rows: 4 KiB)
    assert call(ga=a) == -5 and call(gb=b + 16) == -5 and call(gc=gy) == -5 and call(work=x) == -5
    # nothing to do: accepted without touching a pointer or a device
    assert call(S=0) == 0 and err() == ""
    assert call(stride=0) == 0 and err() == ""
    assert bwd(None, None, None, None, None, None, None, None, None, None, 0, 7, 9, 0, None) == 0
    assert bwd(None, None, None, None, None, None, None, None, None, None, 3, 0, 12, SRC_SHARED, None) == 0


def _shipped():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    return shipped_isa.ShippedLibrary()


def test_shipped_library_has_every_instantiation_without_scratch_and_keeps_the_forward_symbols():
    with _shipped() as lib:
        kernels = lib.kernels
    for log2d in range(6, 13):
        mine = {n: k for n, k in kernels.items() if n.startswith(f"whvi::fused_shs_bwd_kernel<float, {log2d}, ")}
        forms = {re.search(r"<(.*)>", n).group(1).split(", ")[3] for n in mine}            # NT
        assert forms == {"true", "false"}, (log2d, sorted(mine))
        for name, k in mine.items():
            assert k["scratch"] == 0, (name, k)
            assert k["vgprs"] + k["agprs"] <= 512, (name, k)
            if log2d <= 11:
                assert k["vgprs"] + k["agprs"] <= 256, (name, k)        # at least two waves per SIMD below the one-row tile of 4096
    assert any(n.startswith("whvi::fused_shs_bwd_finish_kernel") for n in kernels)
    golden = [g for g in open(os.path.join(ROOT, "tests", "golden", "fused_shs_kernel_symbols_f32_f64.txt")).read().split("\n")
              if g.strip()]
    now = sorted(n for n in kernels if re.match(r"whvi::fused_shs_kernel<(float|double), ", n))
    assert now == sorted(golden), "the float / double instantiations of fused_shs_kernel changed"


def test_flag_is_ignored_on_host_tensors():
    from whvi_amd.fastfood import FastfoodFunction, WHVIFastfoodMatrix
    D, S, B = 64, 3, 5
    for shared in (False, True):
        grads = []
        for flag in (False, True):
            x = torch.randn(B if shared else S * B, D, generator=torch.Generator().manual_seed(1)).requires_grad_()
            a, b, c = (torch.randn(n, generator=torch.Generator().manual_seed(2 + i)).requires_grad_()
                       for i, n in enumerate((D, S * D, D)))
            y = FastfoodFunction.apply(x, a, b.view(S, D), c, S, B, shared, False, flag)
            w = torch.randn(y.shape, generator=torch.Generator().manual_seed(9))
            (y * w).sum().backward()
            grads.append((y.detach(), x.grad, a.grad, b.grad, c.grad))
        for u, v in zip(*grads):
            assert torch.equal(u, v)
    assert WHVIFastfoodMatrix.fused_backward is False
    outs = []
    for flag in (False, True):
        torch.manual_seed(3)
        layer = WHVIFastfoodMatrix(D)
        layer.fused_backward = flag
        x = torch.randn(B, D, generator=torch.Generator().manual_seed(4)).requires_grad_()
        loss = layer.forward_mc(x, S).square().sum()
        loss.backward()
        outs.append([loss.detach(), x.grad] + [p.grad for p in layer.parameters()])
    for u, v in zip(*outs):
        assert torch.equal(u, v)
