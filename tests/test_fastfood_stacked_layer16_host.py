"""The rectangular fastfood layer on 16-bit activations with its bias, its neighbouring ReLUs and its narrowing in the one launch
(whvi_fused_shs_stacked_layer_f16 / _bf16, whvi_amd.fastfood.FastfoodStackedLayer16Function,
``WHVIFastfoodStackedMatrix.fused_epilogue16``) as far as it can be checked without a GPU: the ABI declares and exports the
three symbols, the support rule and its Python mirror, every refusal and its precedence for both entries (ctypes with fake
aligned pointers: the checks happen before any device call; extents for 2-byte activations and 4-byte vectors, n_cols and
ld_dst in whole 8-column chunks), what the shipped library contains -- a fused_stacked16_layer_kernel<T, L, fused_bwd_k(L, 8),
NT> for both storage types, every L in 6 .. 11 and both NT, none with scratch -- and, on host tensors, that the flags change
nothing: no folding, the same values and gradients, no launch named."""
import ctypes
import os
import re

import pytest
import torch

import test_fastfood_stacked_host as stacked_host
from test_fastfood_stacked_host import ROOT, make_layer

ENTRIES = ("whvi_fused_shs_stacked_layer16_supported", "whvi_fused_shs_stacked_layer_f16", "whvi_fused_shs_stacked_layer_bf16")
SRC_SHARED, RELU_IN, RELU_OUT = 4, 16, 32
ARG, SIZE, ALIGN, OVERLAP = -1, -2, -3, -5


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
    # no new flag bit: the three the float32 layer entry takes
    bits = {name: int(value) for name, value in re.findall(r"#define (WHVI_FUSED_[A-Z_]+)\s+(\d+)", raw)}
    assert sorted(bits.values()) == [1, 2, 4, 8, 16, 32]
    assert bits["WHVI_FUSED_RELU_IN"] == RELU_IN and bits["WHVI_FUSED_RELU_OUT"] == RELU_OUT and bits["WHVI_FUSED_SRC_SHARED"] == SRC_SHARED


def test_support_rule_and_its_mirror():
    from whvi_amd import _hip
    L = _hip.lib()
    for log2d in range(5, 13):
        for J in range(0, 87):
            for has_bias in (0, 1):
                rule = 6 <= log2d <= 11 and J >= 1 and (12 + 4 * has_bias) * (1 << log2d) * J <= 65536
                assert L.whvi_fused_shs_stacked_layer16_supported(log2d, J, has_bias) == int(rule), (log2d, J, has_bias)
                for dtype in (torch.float16, torch.bfloat16):
                    assert _hip.fused_shs_stacked_layer16_supported(dtype, 1 << log2d, J, bool(has_bias)) == rule, (dtype, log2d, J)
                for dtype in (torch.float32, torch.float64):
                    assert not _hip.fused_shs_stacked_layer16_supported(dtype, 1 << log2d, J, bool(has_bias)), (dtype, log2d, J)
    # with a bias: J <= 4 at D = 1024, J <= 2 at D = 2048
    assert L.whvi_fused_shs_stacked_layer16_supported(10, 4, 1) == 1 and L.whvi_fused_shs_stacked_layer16_supported(10, 5, 1) == 0
    assert L.whvi_fused_shs_stacked_layer16_supported(10, 5, 0) == 1
    assert L.whvi_fused_shs_stacked_layer16_supported(11, 2, 1) == 1 and L.whvi_fused_shs_stacked_layer16_supported(11, 3, 1) == 0
    assert L.whvi_fused_shs_stacked_layer16_supported(9, -1, 0) == 0 and L.whvi_fused_shs_stacked_layer16_supported(9, 1 << 40, 0) == 0
    assert not _hip.fused_shs_stacked_layer16_supported(torch.float16, 100, 2, False)
    # the float32 layer's predicate keeps refusing 16-bit storage
    for dtype in (torch.float16, torch.bfloat16):
        assert not _hip.fused_shs_stacked_layer_supported(dtype, 256, 2, True)


@pytest.mark.parametrize("entry", ENTRIES[1:])
def test_refusals_before_any_device_call_and_their_precedence(entry):
    from whvi_amd import _hip
    fn = getattr(_hip.lib(), entry)
    buf = (ctypes.c_char * (1 << 20))()
    p = (ctypes.addressof(buf) + 15) & ~15
    K = 65536         # J = 2, S = 2, stride = 2, D = 512: dst 8 KiB at ld_dst = 1024, src 4 KiB (2 shared), a / c / bias 4 KiB, b 8 KiB
    dst, src, a, b, c, bias = (p + i * K for i in range(6))

    def call(dst=dst, src=src, a=a, b=b, c=c, bias=bias, J=2, S=2, stride=2, log2d=9, n_cols=1024, ld_dst=None, flags=0):
        return fn(dst, src, a, b, c, bias, J, S, stride, log2d, n_cols, n_cols if ld_dst is None else ld_dst, flags, None)

    err = _hip.last_error
    for flags in (0, SRC_SHARED, RELU_IN, RELU_OUT, SRC_SHARED | RELU_IN | RELU_OUT):       # (accepted: S = 0 launches nothing)
        assert call(S=0, flags=flags) == 0 and err() == "", flags
    # WHVI_ERR_ARG: unknown flags, negative sizes, a null pointer other than bias
    for flags in (1, 2, 8, 64, SRC_SHARED | 8, RELU_IN | RELU_OUT | 128, -1):
        assert call(flags=flags) == ARG and "unknown fused flags" in err(), flags
    for name in ("J", "S", "stride", "n_cols", "ld_dst"):
        assert call(**{name: -8}) == ARG and "negative" in err(), name
    for name in ("dst", "src", "a", "b", "c"):
        assert call(**{name: None}) == ARG and "null" in err(), name
    assert call(bias=None, S=0) == 0
    # WHVI_ERR_SIZE: the support rule ...
    for log2d in (-1, 0, 5, 12, 13):
        assert call(log2d=log2d) == SIZE and "supported range" in err(), log2d
    assert call(J=0, n_cols=0) == SIZE
    assert call(J=9, n_cols=9 * 512) == SIZE and "LDS" in err()                   # 16 * 512 * 9 > 65536 with a bias
    assert call(J=8, n_cols=8 * 512, S=0) == 0                                    # 16 * 512 * 8 = 65536
    assert call(J=10, n_cols=10 * 512, S=0) == SIZE                               # ... which 12 * 512 * 10 fits without one
    assert call(J=10, n_cols=10 * 512, S=0, bias=None) == 0
    assert call(J=11, n_cols=11 * 512, bias=None) == SIZE and "LDS" in err()
    assert call(log2d=10, J=5, n_cols=5120) == SIZE and call(log2d=11, J=3, n_cols=6144) == SIZE
    # ... n_cols and ld_dst: whole 8-column chunks
    for n_cols in (1020, 1022, 1023, 1021, 516):                                  # (1020 = J D - 4: a multiple of 4 is not enough)
        assert call(n_cols=n_cols, ld_dst=1024) == SIZE and "multiples of 8" in err(), n_cols
    assert call(ld_dst=1028) == SIZE and "multiples of 8" in err()
    assert call(ld_dst=1026) == SIZE and "multiples of 8" in err()
    assert call(n_cols=512) == SIZE and "last of the" in err()                    # n_cols = (J - 1) D: the last block would be empty
    assert call(n_cols=1032) == SIZE and "last of the" in err()                   # n_cols = J D + 8
    assert call(n_cols=0) == SIZE and call(n_cols=504) == SIZE
    assert call(n_cols=520, S=0) == 0 and call(n_cols=1016, S=0) == 0
    assert call(n_cols=1024, ld_dst=1016) == SIZE and "ld_dst" in err()           # ld_dst < n_cols
    assert call(n_cols=520, ld_dst=512) == SIZE and "ld_dst" in err()
    assert call(S=1 << 20, stride=1 << 12) == SIZE and "32 bits" in err()
    # WHVI_ERR_ALIGN: every pointer, the bias included
    for name, ptr in (("dst", dst), ("src", src), ("a", a), ("b", b), ("c", c), ("bias", bias)):
        for off in (2, 4, 8):
            assert call(**{name: ptr + off}) == ALIGN and "aligned" in err(), (name, off)
    # WHVI_ERR_OVERLAP: the rows * ld_dst span of dst in 2-byte elements (8 KiB at ld_dst = 1024) over each input: src 4 KiB of
    # 2-byte elements, a, c and the bias 4 KiB and b 8 KiB of floats
    assert call(dst=src) == OVERLAP and "overlap" in err()
    assert call(dst=src + 4096 - 16) == OVERLAP and call(dst=src - 8192 + 16) == OVERLAP
    assert call(dst=a + 4080) == OVERLAP and call(dst=b + 8176) == OVERLAP and call(dst=c - 16) == OVERLAP
    assert call(dst=bias + 4080) == OVERLAP and call(dst=bias - 8192 + 16) == OVERLAP
    assert call(dst=src + 2048 - 16, flags=SRC_SHARED) == OVERLAP                 # (a shared source is sample_stride rows: 2 KiB)
    # the span is rows * ld_dst, not rows * n_cols: 4 rows of pitch 2048 reach 16 KiB
    assert call(dst=src - 16384 + 16, ld_dst=2048) == OVERLAP
    # precedence, in whvi_fused_shs_stacked_layer_f32's order: flags, negative sizes, the sizes, nothing to do, null, 32-bit
    # rows, alignment, overlap
    assert call(flags=64, J=-1) == ARG and "unknown fused flags" in err()
    assert call(J=-1, log2d=12) == ARG and "negative" in err()
    assert call(log2d=12, n_cols=1020) == SIZE and "supported range" in err()
    assert call(J=9, n_cols=1020) == SIZE and "LDS" in err()
    assert call(n_cols=1020, ld_dst=1016) == SIZE and "multiples of 8" in err()
    assert call(n_cols=512, ld_dst=504) == SIZE and "last of the" in err()
    assert call(n_cols=1020, S=0) == SIZE and call(n_cols=1020, dst=None) == SIZE
    assert call(dst=None, S=1 << 20, stride=1 << 12) == ARG and "null" in err()
    assert call(S=1 << 20, stride=1 << 12, src=src + 4) == SIZE and "32 bits" in err()
    assert call(dst=src + 4) == ALIGN
    assert call(bias=bias + 4, dst=bias) == ALIGN
    # nothing to do: accepted without touching a pointer or a device
    assert call(S=0) == 0 and err() == ""
    assert call(stride=0) == 0 and err() == ""
    assert fn(None, None, None, None, None, None, 2, 0, 7, 9, 1024, 1024, 0, None) == 0
    assert fn(None, None, None, None, None, None, 1, 3, 0, 11, 2048, 4096, SRC_SHARED | RELU_OUT, None) == 0


def test_shipped_library_has_the_twenty_four_instantiations():
    with stacked_host._shipped() as lib:
        kernels = lib.kernels
    mine = {n: k for n, k in kernels.items() if "fused_stacked16_layer_kernel<" in n}
    k_of = {6: 2, 7: 2, 8: 2, 9: 2, 10: 2, 11: 4}                           # fused_bwd_k(L, 8)
    want = {f"whvi::fused_stacked16_layer_kernel<{t}, {L}, {k_of[L]}, {nt}>" for t in ("__half", "__hip_bfloat16")
            for L in range(6, 12) for nt in ("true", "false")}
    assert set(mine) == want and len(want) == 24
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgprs"] + k["agprs"] <= 256, (name, k)
        # the substrings by which the sibling kernels' symbol sets are pinned
        assert not any(s in name for s in ("fused_stacked16_kernel<", "fused_shs_", "stacked_bwd16")), name


# ---- the Module on host tensors: the composed route with the flags off and on ------------------------------------------------
def _set_flags(sub, flag16):
    sub.keep_half, sub.fused_epilogue, sub.fused_epilogue16 = True, True, flag16


def _pass(layer, x, S, relu_in, relu_out, flag16):
    sub = layer.weight_submodule
    _set_flags(sub, flag16)
    assert not sub.fuses_relu(x) and not layer.fuses_relu(x)
    x = x.clone().requires_grad_()
    layer.zero_grad()
    torch.manual_seed(21)
    y = layer.forward_mc(x, S, relu_in=relu_in, relu_out=relu_out)
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(22)).to(y.dtype)
    (y * w).sum().backward()
    return y.detach(), x.grad, [p.grad.clone() for p in layer.parameters()]


def test_fuses_relu_is_false_on_host_tensors_with_all_three_flags():
    layer = make_layer(16, 40, bias=True)
    sub = layer.weight_submodule
    assert type(sub).fused_epilogue16 is False
    _set_flags(sub, True)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        for x in (torch.zeros(5, 16, dtype=dtype), torch.zeros(3, 5, 16, dtype=dtype)):
            assert not sub.fuses_relu(x) and not layer.fuses_relu(x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n_in,n_out", [(16, 40), (10, 16)])
def test_the_flag_changes_nothing_on_host_tensors(n_in, n_out, dtype, monkeypatch):
    from whvi_amd import _hip
    S, B = 3, 5

    def no_launch(*args, **kwargs):
        raise AssertionError("a 16-bit launch was called for host tensors")

    for name in ("fused_shs_stacked_layer16", "fused_shs_stacked16", "fused_shs_stacked_layer"):
        monkeypatch.setattr(_hip, name, no_launch)
    layer = make_layer(n_in, n_out, bias=True)
    gen = torch.Generator().manual_seed(9)
    before = _hip.last_kernel()
    for x in (torch.randn(B, n_in, generator=gen).to(dtype), torch.randn(S, B, n_in, generator=gen).to(dtype)):
        for relu_in in (False, True):
            for relu_out in (False, True):
                y0, gx0, gp0 = _pass(layer, x, S, relu_in, relu_out, False)
                y1, gx1, gp1 = _pass(layer, x, S, relu_in, relu_out, True)
                assert y0.shape == (S, B, n_out) and y0.dtype == y1.dtype
                assert gx0.dtype == dtype and gx1.dtype == dtype
                assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
                assert len(gp0) == len(gp1) == 4 * layer.weight_submodule.stack + 1
                for p, q in zip(gp0, gp1):
                    assert torch.equal(p, q)
                assert relu_out is False or bool((y0 >= 0).all())
    assert _hip.last_kernel() == before                                     # (no launch was named by any of these passes)
