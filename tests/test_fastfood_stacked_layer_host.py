"""The rectangular fastfood layer with its bias, its neighbouring ReLUs and its narrowing in the one launch
(whvi_fused_shs_stacked_layer_f32, whvi_amd.fastfood.FastfoodStackedLayerFunction, ``WHVIFastfoodStackedMatrix.fused_epilogue``)
as far as it can be checked without a GPU: the ABI declares and exports the two symbols, the support rule and its Python
mirror, every refusal and its precedence (ctypes with fake aligned pointers: the checks happen before any device call), what
the shipped library contains -- a fused_shs_stacked_layer_kernel<float, L, K, NT> for every L in 6 .. 11 and both NT, none with
scratch, beside the unchanged pinned symbol sets -- and, on host tensors, that the flag changes nothing: the composed route
either way, the same values and gradients for ``forward_mc(x, S, relu_in=, relu_out=)`` and for a whole network's loss."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from whvi_amd.layers import WHVILinear
from whvi_amd.networks import WHVIRegression

import test_fastfood_stacked_host as stacked_host
from test_fastfood_stacked_host import MODE, ROOT, make_layer

ENTRIES = ("whvi_fused_shs_stacked_layer_supported", "whvi_fused_shs_stacked_layer_f32")
SRC_SHARED, RELU_IN, RELU_OUT = 4, 16, 32
ARG, SIZE, ALIGN, OVERLAP = -1, -2, -3, -5


def test_header_declares_and_library_exports_both_symbols():
    from whvi_amd import _hip
    raw = open(os.path.join(ROOT, "include", "whvi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(whvi_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in declared, name
        assert hasattr(lib, name), name
    # the two new flags collide with no other WHVI_FUSED_* bit
    bits = {name: int(value) for name, value in re.findall(r"#define (WHVI_FUSED_[A-Z_]+)\s+(\d+)", raw)}
    assert bits["WHVI_FUSED_RELU_IN"] == RELU_IN == _hip.FUSED_RELU_IN and bits["WHVI_FUSED_RELU_OUT"] == RELU_OUT == _hip.FUSED_RELU_OUT
    assert len(set(bits.values())) == len(bits) and all(v & (v - 1) == 0 for v in bits.values())


def test_support_rule_and_its_mirror():
    from whvi_amd import _hip
    L = _hip.lib()
    for log2d in range(5, 13):
        for J in range(0, 87):
            for has_bias in (0, 1):
                rule = 6 <= log2d <= 11 and J >= 1 and (12 + 4 * has_bias) * (1 << log2d) * J <= 65536
                assert L.whvi_fused_shs_stacked_layer_supported(log2d, J, has_bias) == int(rule), (log2d, J, has_bias)
                assert _hip.fused_shs_stacked_layer_supported(torch.float32, 1 << log2d, J, bool(has_bias)) == rule, (log2d, J, has_bias)
    # with a bias: J <= 4 at D = 1024, J <= 2 at D = 2048
    assert L.whvi_fused_shs_stacked_layer_supported(10, 4, 1) == 1 and L.whvi_fused_shs_stacked_layer_supported(10, 5, 1) == 0
    assert L.whvi_fused_shs_stacked_layer_supported(10, 5, 0) == 1
    assert L.whvi_fused_shs_stacked_layer_supported(11, 2, 1) == 1 and L.whvi_fused_shs_stacked_layer_supported(11, 3, 1) == 0
    assert L.whvi_fused_shs_stacked_layer_supported(9, -1, 0) == 0 and L.whvi_fused_shs_stacked_layer_supported(9, 1 << 40, 0) == 0
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        assert not _hip.fused_shs_stacked_layer_supported(dtype, 256, 2, True)
    assert not _hip.fused_shs_stacked_layer_supported(torch.float32, 100, 2, False)


def test_refusals_before_any_device_call_and_their_precedence():
    from whvi_amd import _hip
    fn = _hip.lib().whvi_fused_shs_stacked_layer_f32
    buf = (ctypes.c_char * (1 << 20))()
    p = (ctypes.addressof(buf) + 15) & ~15
    K = 65536         # J = 2, S = 2, stride = 2, D = 512: dst 16 KiB at ld_dst = 1024, src 8 KiB (4 shared), a / c / bias 4 KiB, b 8 KiB
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
        assert call(**{name: -4}) == ARG and "negative" in err(), name
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
    # ... n_cols and ld_dst
    for n_cols in (1022, 1023, 1021):
        assert call(n_cols=n_cols) == SIZE and "multiples of 4" in err(), n_cols
    assert call(ld_dst=1026) == SIZE and "multiples of 4" in err()
    assert call(n_cols=512) == SIZE and "last of the" in err()                    # n_cols = (J - 1) D: the last block would be empty
    assert call(n_cols=1028) == SIZE and "last of the" in err()                   # n_cols = J D + 4
    assert call(n_cols=0) == SIZE and call(n_cols=508) == SIZE
    assert call(n_cols=516, S=0) == 0 and call(n_cols=1020, S=0) == 0
    assert call(n_cols=1024, ld_dst=1020) == SIZE and "ld_dst" in err()           # ld_dst < n_cols
    assert call(n_cols=516, ld_dst=512) == SIZE and "ld_dst" in err()
    assert call(S=1 << 20, stride=1 << 12) == SIZE and "32 bits" in err()
    # WHVI_ERR_ALIGN: every pointer, the bias included
    for name, ptr in (("dst", dst), ("src", src), ("a", a), ("b", b), ("c", c), ("bias", bias)):
        assert call(**{name: ptr + 4}) == ALIGN and "aligned" in err(), name
    # WHVI_ERR_OVERLAP: the rows * ld_dst span of dst (16 KiB at ld_dst = 1024) over each input
    assert call(dst=src) == OVERLAP and "overlap" in err()
    assert call(dst=src + 8192 - 16) == OVERLAP and call(dst=src - 16384 + 16) == OVERLAP
    assert call(dst=a + 4080) == OVERLAP and call(dst=b + 8176) == OVERLAP and call(dst=c - 16) == OVERLAP
    assert call(dst=bias + 4080) == OVERLAP and call(dst=bias - 16384 + 16) == OVERLAP
    assert call(dst=src + 4096 - 16, flags=SRC_SHARED) == OVERLAP                 # (a shared source is sample_stride rows: 4 KiB)
    # the span is rows * ld_dst, not rows * n_cols: 4 rows of pitch 2048 reach 32 KiB
    assert call(dst=src - 32768 + 16, ld_dst=2048) == OVERLAP
    # precedence, in whvi_fused_shs_stacked_f32's order: flags, negative sizes, the sizes, nothing to do, null, 32-bit rows,
    # alignment, overlap
    assert call(flags=64, J=-1) == ARG and "unknown fused flags" in err()
    assert call(J=-1, log2d=12) == ARG and "negative" in err()
    assert call(log2d=12, n_cols=1022) == SIZE and "supported range" in err()
    assert call(J=9, n_cols=1022) == SIZE and "LDS" in err()
    assert call(n_cols=1022, ld_dst=1020) == SIZE and "multiples of 4" in err()
    assert call(n_cols=512, ld_dst=508) == SIZE and "last of the" in err()
    assert call(n_cols=1022, S=0) == SIZE and call(n_cols=1022, dst=None) == SIZE
    assert call(dst=None, S=1 << 20, stride=1 << 12) == ARG and "null" in err()
    assert call(S=1 << 20, stride=1 << 12, src=src + 4) == SIZE and "32 bits" in err()
    assert call(dst=src + 4) == ALIGN
    # nothing to do: accepted without touching a pointer or a device
    assert call(S=0) == 0 and err() == ""
    assert call(stride=0) == 0 and err() == ""
    assert fn(None, None, None, None, None, None, 2, 0, 7, 9, 1024, 1024, 0, None) == 0
    assert fn(None, None, None, None, None, None, 1, 3, 0, 11, 2048, 4096, SRC_SHARED | RELU_OUT, None) == 0


def test_shipped_library_has_the_twelve_instantiations_and_keeps_the_pinned_symbol_sets():
    with stacked_host._shipped() as lib:
        kernels = lib.kernels
    mine = {n: k for n, k in kernels.items() if n.startswith("whvi::fused_shs_stacked_layer_kernel<")}
    want = {f"whvi::fused_shs_stacked_layer_kernel<float, {L}, {8 if L == 11 else 4}, {nt}>" for L in range(6, 12) for nt in ("true", "false")}
    assert set(mine) == want and len(want) == 12
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgprs"] + k["agprs"] <= 256, (name, k)
    # whvi::fused_shs_stacked_kernel<, whvi::fused_shs_kernel<(float|double) and whvi::fused_shs_bwd_kernel<: as they were
    stacked_host.test_shipped_library_has_every_instantiation_and_keeps_the_pinned_symbol_sets()


# ---- the Module on host tensors: the composed route with the flag off and on -------------------------------------------------
def _pass(layer, x, S, relu_in, relu_out, flag):
    sub = layer.weight_submodule
    sub.fused_epilogue = flag
    assert not sub.fuses_relu(x) and not layer.fuses_relu(x)
    x = x.clone().requires_grad_()
    layer.zero_grad()
    torch.manual_seed(21)
    y = layer.forward_mc(x, S, relu_in=relu_in, relu_out=relu_out)
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(22))
    (y * w).sum().backward()
    return y.detach(), x.grad, [p.grad.clone() for p in layer.parameters()]


@pytest.mark.parametrize("n_in,n_out", [(16, 40), (10, 16)])
def test_the_flag_changes_nothing_on_host_tensors(n_in, n_out):
    S, B = 3, 5
    layer = make_layer(n_in, n_out, bias=True)
    assert type(layer.weight_submodule).fused_epilogue is False
    gen = torch.Generator().manual_seed(9)
    for x in (torch.randn(B, n_in, generator=gen), torch.randn(S, B, n_in, generator=gen)):
        for relu_in in (False, True):
            for relu_out in (False, True):
                y0, gx0, gp0 = _pass(layer, x, S, relu_in, relu_out, False)
                y1, gx1, gp1 = _pass(layer, x, S, relu_in, relu_out, True)
                assert y0.shape == (S, B, n_out)
                assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
                assert len(gp0) == len(gp1) == 4 * layer.weight_submodule.stack + 1
                for p, q in zip(gp0, gp1):
                    assert torch.equal(p, q)
                # ... and they are relu(layer(relu(x))) of the plain call under the same seed
                torch.manual_seed(21)
                with torch.no_grad():
                    plain = layer.forward_mc(torch.relu(x) if relu_in else x, S)
                assert torch.equal(y0, torch.relu(plain) if relu_out else plain)
                assert relu_out is False or bool((y0 >= 0).all())


def test_network_loss_and_gradients_with_the_flag_on_every_stacked_layer():
    def run(flag):
        torch.manual_seed(0)
        net = WHVIRegression([WHVILinear(6, 16, lambda_=1.0, mode=MODE), nn.ReLU(), WHVILinear(16, 32, lambda_=1.0, mode=MODE), nn.ReLU(),
                              WHVILinear(32, 2, lambda_=1.0, mode=MODE)], train_samples=3, eval_samples=5)
        x, y = torch.randn(12, 6), torch.randn(12, 2)
        stacked = [m.weight_submodule for m in net.modules() if isinstance(m, WHVILinear)]
        assert len(stacked) == 3 and all(type(s).__name__ == "WHVIFastfoodStackedMatrix" for s in stacked)
        for s in stacked:
            s.fused_epilogue = flag
        net.mc_mode = "batched"
        net.train()
        net.zero_grad()
        torch.manual_seed(1)
        loss = net.loss(x, y, n=100)
        loss.backward()
        return loss.detach(), [p.grad.clone() for p in net.parameters()]

    loss0, grads0 = run(False)
    loss1, grads1 = run(True)
    assert torch.isfinite(loss0) and torch.equal(loss0, loss1)
    assert len(grads0) == len(grads1) > 0
    for p, q in zip(grads0, grads1):
        assert torch.equal(p, q)
