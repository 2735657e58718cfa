"""The one-launch backward of the rectangular fastfood layer with its epilogue (whvi_fused_shs_stacked_layer_bwd_f32,
``FastfoodStackedLayerFunction(..., fused_backward=True, fused_epilogue_backward=True)``) as far as it can be checked without a
GPU: the ABI declares and exports the three symbols, the support rule and its Python mirror, the workspace query against a
restatement of ``fused_bwd_geom``, every refusal and its precedence (ctypes with fake aligned pointers: the checks happen before
any device call), what the shipped library contains -- the 64 ``fused_shs_stacked_layer_bwd_kernel<float, L, K, J, bias, nt>``
instantiations, none with scratch, beside the unchanged pinned symbol sets -- and, on host tensors, that the flag changes
nothing."""
import ctypes
import os
import re

import pytest
import torch

import test_fastfood_stacked_host as stacked_host
from test_fastfood_stacked_host import ROOT, make_layer
from test_fastfood_stacked_bwd_host import _n_slabs

ENTRIES = ("whvi_fused_shs_stacked_layer_bwd_supported", "whvi_fused_shs_stacked_layer_bwd_workspace",
           "whvi_fused_shs_stacked_layer_bwd_f32")
SRC_SHARED, RELU_IN, RELU_OUT = 4, 16, 32
ARG, SIZE, ALIGN, OVERLAP = -1, -2, -3, -5


def _rule(log2d, J, has_bias):
    return (6 <= log2d <= 10 and 2 <= J <= 4) or (log2d == 11 and J == 2)


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
    n_yes = 0
    for log2d in range(5, 13):
        for J in range(0, 7):
            for has_bias in (0, 1):
                want = _rule(log2d, J, has_bias)
                n_yes += want
                assert L.whvi_fused_shs_stacked_layer_bwd_supported(log2d, J, has_bias) == int(want), (log2d, J, has_bias)
                assert _hip.fused_shs_stacked_layer_bwd_supported(torch.float32, 1 << log2d, J, bool(has_bias)) == want
                # never more than the backward it starts from
                assert not want or L.whvi_fused_shs_stacked_bwd_supported(log2d, J) == 1
    assert n_yes == 32                                     # times the two cache policies: the 64 shipped kernels
    for log2d, J in ((-1, 2), (0, 2), (9, -1), (9, 1 << 40), (13, 2), (40, 2)):
        assert L.whvi_fused_shs_stacked_layer_bwd_supported(log2d, J, 1) == 0, (log2d, J)
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        assert not _hip.fused_shs_stacked_layer_bwd_supported(dtype, 256, 2, True)
    assert not _hip.fused_shs_stacked_layer_bwd_supported(torch.float32, 100, 2, False)
    assert not _hip.fused_shs_stacked_layer_bwd_supported(torch.float32, 0, 2, False)


def test_workspace_query():
    from whvi_amd import _hip
    L = _hip.lib()
    q = L.whvi_fused_shs_stacked_layer_bwd_workspace
    for S, stride, log2d, J in ((1, 1, 6, 2), (3, 5, 6, 4), (2, 777, 7, 3), (4, 64, 8, 2), (16, 8192, 10, 4), (64, 1000, 7, 4),
                                (16, 4096, 11, 2), (1, 256, 10, 4), (2000, 3, 9, 3), (8, 4096, 10, 4)):
        D = 1 << log2d
        n_slabs = _n_slabs(S, stride, log2d)
        for has_bias in (0, 1):
            assert q(S, stride, log2d, J, has_bias) == S * n_slabs * (12 + 4 * has_bias) * D * J, (S, stride, log2d, J, has_bias)
        # without a bias the slots are those of the backward without the epilogue
        assert q(S, stride, log2d, J, 0) == L.whvi_fused_shs_stacked_bwd_workspace(S, stride, log2d, J)
    for S, stride in ((0, 7), (7, 0), (0, 0)):
        assert q(S, stride, 9, 2, 1) == 0
    assert q(-1, 4, 9, 2, 0) == ARG and q(4, -1, 9, 2, 0) == ARG and q(4, 4, 9, -1, 1) == ARG
    for log2d, J in ((5, 2), (12, 2), (11, 3), (9, 0), (9, 1), (9, 5), (-1, 2)):
        assert q(4, 4, log2d, J, 1) == SIZE, (log2d, J)
        assert q(0, 0, log2d, J, 0) == SIZE, (log2d, J)


def test_refusals_before_any_device_call():
    from whvi_amd import _hip
    fn = _hip.lib().whvi_fused_shs_stacked_layer_bwd_f32
    buf = (ctypes.c_char * (1 << 20))()
    p = (ctypes.addressof(buf) + 15) & ~15
    K = 65536
    # J = 2, S = 2, stride = 2, D = 512, n_cols = 1000, ld = 1008: grad_y and y 4 rows * 4032 bytes, x 8 KiB (4 shared), a / c
    # 4 KiB, b 8 KiB; grad_x 8 KiB, grad_a / grad_c / grad_bias 4 KiB, grad_b 8 KiB, the workspace 2 blocks * 16 KiB
    names = ("grad_x", "grad_a", "grad_b", "grad_c", "grad_bias", "work", "grad_y", "y", "x", "a", "b", "c")
    ptrs = {name: p + i * K for i, name in enumerate(names)}
    assert _hip.lib().whvi_fused_shs_stacked_layer_bwd_workspace(2, 2, 9, 2, 1) == 2 * 16384

    def call(J=2, S=2, stride=2, log2d=9, n_cols=1000, ld=1008, flags=RELU_IN | RELU_OUT, **over):
        args = dict(ptrs)
        args.update(over)
        if not flags & RELU_OUT and "y" not in over:
            args["y"] = None
        return fn(*(args[n] for n in names), J, S, stride, log2d, n_cols, ld, flags, None)

    err = _hip.last_error
    for flags in (1, 2, 8, 64, SRC_SHARED | 128):
        assert call(flags=flags) == ARG and "unknown fused flags" in err(), flags
    for name in ("J", "S", "stride", "n_cols", "ld"):
        assert call(**{name: -4}) == ARG and "negative" in err(), name
    for log2d in (-1, 0, 5, 12, 13):
        assert call(log2d=log2d) == SIZE and "supported range" in err(), log2d
    for J in (0, 1, 5, 6):
        assert call(J=J, n_cols=512 * J, ld=512 * J) == SIZE and "supported range" in err(), J
    assert call(log2d=11, J=3) == SIZE and call(log2d=11, J=4) == SIZE
    assert call(n_cols=1002) == SIZE and "multiples of 4" in err()
    assert call(ld=1010) == SIZE and "multiples of 4" in err()
    assert call(n_cols=512, ld=512) == SIZE and "last of the" in err()          # n_cols = (J - 1) D
    assert call(n_cols=1028, ld=1028) == SIZE and "last of the" in err()        # n_cols = J D + 4
    assert call(n_cols=1000, ld=996) == SIZE and "below n_cols" in err()        # ld < n_cols
    # precedence: flags, negative sizes, support, multiples of 4, n_cols' range, ld, the empty call, pointers
    assert call(flags=1, J=-1) == ARG and "flags" in err()
    assert call(J=-1, log2d=3) == ARG and call(J=5, n_cols=1002) == SIZE and "supported range" in err()
    assert call(n_cols=1002, ld=996) == SIZE and "multiples of 4" in err()
    assert call(n_cols=512, ld=508) == SIZE and "last of the" in err()
    assert call(ld=996, S=0) == SIZE and call(n_cols=1002, grad_a=None) == SIZE
    # nothing to do: accepted without touching a pointer or a device
    assert call(S=0) == 0 and err() == ""
    assert call(stride=0) == 0 and err() == ""
    assert fn(*([None] * 12), 2, 0, 7, 9, 1024, 1024, 0, None) == 0
    assert fn(*([None] * 12), 4, 3, 0, 10, 4000, 4096, SRC_SHARED | RELU_OUT, None) == 0
    for name in names:
        if name in ("grad_x", "grad_bias", "y"):
            continue
        assert call(**{name: None}) == ARG and "null" in err(), name
    assert call(grad_x=None, grad_bias=None, S=1 << 21, stride=1) == SIZE        # (both optional: on to the limits)
    assert call(y=None) == ARG and "y is given exactly" in err()                # y missing with RELU_OUT
    assert call(flags=RELU_IN, y=ptrs["y"]) == ARG and "y is given exactly" in err()     # y given without it
    assert call(S=1 << 20, stride=1 << 12) == SIZE and "rows are indexed with 32 bits" in err()
    # rows < 2^32 and ld < 2^32, but their product would leave 64 bits in the overlap spans
    assert call(S=1 << 16, stride=1 << 15, ld=(1 << 32) - 4) == SIZE and "rows * ld" in err()
    assert call(ld=1 << 32) == SIZE and "beyond 32 bits" in err()
    # 2 * (S + 3) * 512 >= 2^31 with a bias, 2 * (S + 2) * 512 without
    big = (1 << 21) - 3
    assert call(S=big, stride=1) == SIZE and "gradients are indexed with 32 bits" in err()
    assert call(S=big, stride=1, grad_bias=None) == OVERLAP                     # (past the limit: b and grad_b span everything)
    assert call(S=big + 1, stride=1, grad_bias=None) == SIZE and "gradients" in err()
    for name in names:
        assert call(**{name: ptrs[name] + 4}) == ALIGN and "aligned" in err(), name
    # null before the limits before alignment
    assert call(a=None, x=ptrs["x"] + 4) == ARG and call(S=1 << 21, stride=1, x=ptrs["x"] + 4) == SIZE
    assert call(y=None, x=ptrs["x"] + 4) == ARG
    # every output and the workspace over every input, y included (first and last 16 bytes); grad_y and y span rows * ld
    span = 4 * 1008 * 4
    size_in = {"grad_y": span, "y": span, "x": 8192, "a": 4096, "b": 8192, "c": 4096}
    size_out = {"grad_x": 8192, "grad_a": 4096, "grad_b": 8192, "grad_c": 4096, "grad_bias": 4096, "work": 32768}
    for o, ob in size_out.items():
        for i, ib in size_in.items():
            assert call(**{o: ptrs[i]}) == OVERLAP and "overlap" in err(), (o, i)
            assert call(**{o: ptrs[i] + ib - 16}) == OVERLAP, (o, i)
            assert call(**{o: ptrs[i] - ob + 16}) == OVERLAP, (o, i)
    assert call(grad_x=ptrs["y"]) == OVERLAP                                     # y overlapping grad_x
    assert call(a=ptrs["work"] + 32768 - 16) == OVERLAP                          # (the slots are 16 KiB each with a bias)
    assert call(grad_x=ptrs["x"] + 4096 - 16, flags=SRC_SHARED | RELU_OUT) == OVERLAP    # (a shared x is sample_stride rows)
    # the gap columns of the last row count: the span is rows * ld, not rows * n_cols
    assert call(grad_a=ptrs["grad_y"] + span - 16) == OVERLAP and call(grad_a=ptrs["y"] + span - 16) == OVERLAP


def test_shipped_library_has_the_64_instantiations_and_keeps_the_pinned_symbol_sets():
    with stacked_host._shipped() as lib:
        kernels = lib.kernels
    mine = {n: k for n, k in kernels.items() if n.startswith("whvi::fused_shs_stacked_layer_bwd_kernel<")}
    want = {f"whvi::fused_shs_stacked_layer_bwd_kernel<float, {L}, {8 if L == 11 else 4}, {J}, {bias}, {nt}>"
            for L in range(6, 12) for J in range(2, 5) for b, bias in enumerate(("false", "true")) if _rule(L, J, b)
            for nt in ("true", "false")}
    assert len(want) == 64 and set(mine) == want
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert max(k["vgprs"], k["vgprs"] + k["agprs"]) <= 512, (name, k)
    assert len([n for n in kernels if "fused_shs_stacked_layer_bwd_finish_kernel" in n]) == 1
    # whvi::fused_shs_kernel<(float|double), whvi::fused_shs_bwd_kernel<, whvi::fused_shs_stacked_kernel<: as they were
    stacked_host.test_shipped_library_has_every_instantiation_and_keeps_the_pinned_symbol_sets()
    # ... and so are the backward without the epilogue and the forward with it
    bwd = {f"whvi::fused_shs_stacked_bwd_kernel<float, {L}, {8 if L == 11 else 4}, {J}, {nt}>"
           for L in range(6, 12) for J in range(2, 5) if _rule(L, J, 0) for nt in ("true", "false")}
    assert {n for n in kernels if n.startswith("whvi::fused_shs_stacked_bwd_kernel<")} == bwd and len(bwd) == 32
    fwd = {f"whvi::fused_shs_stacked_layer_kernel<float, {L}, {8 if L == 11 else 4}, {nt}>" for L in range(6, 12) for nt in ("true", "false")}
    assert {n for n in kernels if n.startswith("whvi::fused_shs_stacked_layer_kernel<")} == fwd


# ---- the Module on host tensors: the composed backward with the flag off and on ----------------------------------------------
def _pass(layer, x, S, relu_in, relu_out, flag):
    sub = layer.weight_submodule
    sub.fused_epilogue = sub.fused_backward = sub.fused_epilogue_backward = flag
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
    assert type(layer.weight_submodule).fused_epilogue_backward is False
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
