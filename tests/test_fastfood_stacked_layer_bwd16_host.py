"""The one-launch backward of the rectangular fastfood layer with its epilogue on 16-bit activations
(whvi_fused_shs_stacked_layer_bwd_f16 / _bf16, ``FastfoodStackedLayer16Function(..., fused_backward=True, fused_backward16=True,
fused_epilogue_backward16=True)``) as far as it can be checked without a GPU: the ABI declares and exports the three symbols, the
support rule and its Python mirror, every refusal and its precedence for both entries (ctypes with fake aligned pointers: the
checks happen before any device call; the extents of grad_x, grad_y, y and x are counted in 2-byte elements, n_cols and ld in
whole 8-column chunks), what the shipped library contains -- the 128 ``fused_layer_bwd16_kernel<__half | __hip_bfloat16, L, K, J,
bias, nt>`` instantiations, none with scratch, one new finishing kernel, and the unchanged pinned symbol sets -- the case list of
tools/layer_bwd16_table.py, and that on host tensors the new flag changes nothing.

The overlap check at 2 bytes per element is decided here from the refusing side: a range that reaches into the last 16 bytes of
a 2-byte extent is refused.  The accepting side needs a launch, so it is in tests/test_fastfood_stacked_layer_bwd16_gpu.py
(``grad_x`` directly behind the ``rows * ld`` span of ``y`` in one buffer)."""
import ctypes
import os
import re
import sys

import pytest
import torch

import test_fastfood_stacked_host as stacked_host
from test_fastfood_stacked_host import ROOT, make_layer

sys.path.insert(0, os.path.join(ROOT, "tools"))
ENTRIES = ("whvi_fused_shs_stacked_layer_bwd16_supported", "whvi_fused_shs_stacked_layer_bwd_f16",
           "whvi_fused_shs_stacked_layer_bwd_bf16")
TYPES = ("__half", "__hip_bfloat16")
K16 = {6: 2, 7: 2, 8: 2, 9: 2, 10: 2, 11: 4}                               # fused_bwd_k(L, 8)
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
    # no new flag bit: the shared source, the two ReLUs and the older ones
    flags = dict(re.findall(r"#define (WHVI_FUSED_[A-Z_]+)\s+(\d+)", raw))
    assert sorted(int(v) for v in flags.values()) == [1, 2, 4, 8, 16, 32], flags
    assert (_hip.FUSED_SRC_SHARED, _hip.FUSED_RELU_IN, _hip.FUSED_RELU_OUT) == (SRC_SHARED, RELU_IN, RELU_OUT)


def test_support_rule_and_its_mirror():
    from whvi_amd import _hip
    L = _hip.lib()
    n_yes = 0
    for log2d in range(5, 13):
        for J in range(0, 7):
            for has_bias in (0, 1):
                want = _rule(log2d, J, has_bias)
                n_yes += want
                assert L.whvi_fused_shs_stacked_layer_bwd16_supported(log2d, J, has_bias) == int(want), (log2d, J, has_bias)
                for dtype in (torch.float16, torch.bfloat16):
                    assert _hip.fused_shs_stacked_layer_bwd16_supported(dtype, 1 << log2d, J, bool(has_bias)) == want
                for dtype in (torch.float32, torch.float64):
                    assert not _hip.fused_shs_stacked_layer_bwd16_supported(dtype, 1 << log2d, J, bool(has_bias))
                # never more than the 16-bit backward it starts from, and the float32 entry's workspace serves it
                assert not want or L.whvi_fused_shs_stacked_bwd16_supported(log2d, J) == 1
                assert not want or L.whvi_fused_shs_stacked_layer_bwd_supported(log2d, J, has_bias) == 1
    assert n_yes == 32                                     # times two dtypes and two cache policies: the 128 shipped kernels
    for log2d, J in ((-1, 2), (0, 2), (9, -1), (9, 1 << 40), (13, 2), (40, 2)):
        assert L.whvi_fused_shs_stacked_layer_bwd16_supported(log2d, J, 1) == 0, (log2d, J)
    assert not _hip.fused_shs_stacked_layer_bwd16_supported(torch.float16, 100, 2, False)
    assert not _hip.fused_shs_stacked_layer_bwd16_supported(torch.bfloat16, 0, 2, True)
    # the float32 functions keep refusing 16-bit dtypes
    for dtype in (torch.float16, torch.bfloat16):
        assert not _hip.fused_shs_stacked_layer_bwd_supported(dtype, 256, 2, True)


@pytest.mark.parametrize("sfx", ["f16", "bf16"])
def test_refusals_before_any_device_call_and_their_precedence(sfx):
    from whvi_amd import _hip
    fn = getattr(_hip.lib(), "whvi_fused_shs_stacked_layer_bwd_" + sfx)
    buf = (ctypes.c_char * (1 << 20))()
    p = (ctypes.addressof(buf) + 15) & ~15
    K = 65536
    # J = 2, S = 2, stride = 2, D = 512, n_cols = 1000, ld = 1008: grad_y and y 4 rows * 2016 bytes, x 4 KiB (2 shared), grad_x
    # 4 KiB -- 2-byte elements; a / c 4 KiB, b 8 KiB, grad_a / grad_c / grad_bias 4 KiB, grad_b 8 KiB -- float32; the workspace
    # 2 blocks * 16 KiB
    names = ("grad_x", "grad_a", "grad_b", "grad_c", "grad_bias", "work", "grad_y", "y", "x", "a", "b", "c")
    ptrs = {name: p + (i + 1) * K for i, name in enumerate(names)}
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
        assert call(**{name: -8}) == ARG and "negative" in err(), name
    for log2d in (-1, 0, 5, 12, 13):
        assert call(log2d=log2d) == SIZE and "supported range" in err(), log2d
    for J in (0, 1, 5, 6):
        assert call(J=J, n_cols=512 * J, ld=512 * J) == SIZE and "supported range" in err(), J
    assert call(log2d=11, J=3) == SIZE and call(log2d=11, J=4) == SIZE
    assert call(n_cols=1020, ld=1024) == SIZE and "multiples of 8" in err()     # n_cols = J D - 4: a multiple of 4 only
    assert call(n_cols=1004) == SIZE and "multiples of 8" in err()
    assert call(ld=1004) == SIZE and "multiples of 8" in err()                  # ld not a multiple of 8
    assert call(ld=1012) == SIZE and "multiples of 8" in err()
    assert call(n_cols=512, ld=512) == SIZE and "last of the" in err()          # n_cols = (J - 1) D
    assert call(n_cols=1032, ld=1032) == SIZE and "last of the" in err()        # n_cols = J D + 8
    assert call(n_cols=1000, ld=992) == SIZE and "below n_cols" in err()        # ld < n_cols
    # precedence: flags, negative sizes, support, multiples of 8, n_cols' range, ld, the empty call, pointers
    assert call(flags=1, J=-1) == ARG and "flags" in err()
    assert call(J=-1, log2d=3) == ARG and call(J=5, n_cols=1004) == SIZE and "supported range" in err()
    assert call(n_cols=1004, ld=992) == SIZE and "multiples of 8" in err()
    assert call(n_cols=512, ld=504) == SIZE and "last of the" in err()
    assert call(ld=992, S=0) == SIZE and call(n_cols=1004, grad_a=None) == SIZE
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
    assert call(flags=0, y=ptrs["y"]) == ARG and "y is given exactly" in err()
    assert call(S=1 << 20, stride=1 << 12) == SIZE and "rows are indexed with 32 bits" in err()
    assert call(S=1 << 16, stride=1 << 15, ld=(1 << 32) - 8) == SIZE and "rows * ld" in err()
    assert call(ld=1 << 32) == SIZE and "beyond 32 bits" in err()
    # 2 * (S + 3) * 512 >= 2^31 with a bias, 2 * (S + 2) * 512 without
    big = (1 << 21) - 3
    assert call(S=big, stride=1) == SIZE and "gradients are indexed with 32 bits" in err()
    assert call(S=big + 1, stride=1, grad_bias=None) == SIZE and "gradients" in err()
    for name in names:
        assert call(**{name: ptrs[name] + 4}) == ALIGN and "aligned" in err(), name
        assert call(**{name: ptrs[name] + 2}) == ALIGN and "aligned" in err(), name
    assert call(grad_bias=ptrs["grad_bias"] + 8) == ALIGN and "aligned" in err()         # a misaligned grad_bias
    # null before the limits before alignment before overlap
    assert call(a=None, x=ptrs["x"] + 4) == ARG and call(S=1 << 21, stride=1, x=ptrs["x"] + 4) == SIZE
    assert call(y=None, x=ptrs["x"] + 4) == ARG
    assert call(grad_x=ptrs["x"] + 4) == ALIGN
    # every output and the workspace over every input, y included (first and last 16 bytes); grad_y and y span rows * ld 2-byte
    # elements, x and grad_x rows * D of them
    span = 4 * 1008 * 2
    size_in = {"grad_y": span, "y": span, "x": 4096, "a": 4096, "b": 8192, "c": 4096}
    size_out = {"grad_x": 4096, "grad_a": 4096, "grad_b": 8192, "grad_c": 4096, "grad_bias": 4096, "work": 32768}
    for o, ob in size_out.items():
        for i, ib in size_in.items():
            assert call(**{o: ptrs[i]}) == OVERLAP and "overlap" in err(), (o, i)
            assert call(**{o: ptrs[i] + ib - 16}) == OVERLAP, (o, i)
            assert call(**{o: ptrs[i] - ob + 16}) == OVERLAP, (o, i)
    assert call(grad_x=ptrs["y"]) == OVERLAP                                     # y over grad_x
    assert call(a=ptrs["work"] + 32768 - 16) == OVERLAP                          # (the slots are 16 KiB each with a bias)
    assert call(grad_x=ptrs["x"] + 2048 - 16, flags=SRC_SHARED | RELU_OUT) == OVERLAP    # (a shared x is sample_stride rows: 2 KiB)
    # the gap columns of the last row count: the span is rows * ld, not rows * n_cols, in 2-byte elements
    assert span - 16 > 4 * 1000 * 2
    assert call(grad_a=ptrs["grad_y"] + span - 16) == OVERLAP and call(grad_a=ptrs["y"] + span - 16) == OVERLAP
    assert call(grad_x=None, grad_a=ptrs["grad_y"] - 4096 + 16) == OVERLAP


def test_shipped_library_has_the_128_instantiations_and_keeps_the_pinned_symbol_sets():
    import layer_bwd16_table as tb
    with stacked_host._shipped() as lib:
        kernels = lib.kernels
    mine = {n: k for n, k in kernels.items() if n.startswith("whvi::fused_layer_bwd16_kernel<")}
    want = {f"whvi::fused_layer_bwd16_kernel<{t}, {L}, {K16[L]}, {J}, {bias}, {nt}>"
            for t in TYPES for L in range(6, 12) for J in range(2, 5) for b, bias in enumerate(("false", "true"))
            if _rule(L, J, b) for nt in ("true", "false")}
    assert len(want) == 128 and set(mine) == want
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert max(k["vgprs"], k["vgprs"] + k["agprs"]) <= 512, (name, k)
        # the substrings by which the sibling kernels' symbol sets are pinned
        assert not any(s in name for s in ("fused_shs_", "stacked_bwd16", "fused_stacked16_kernel<",
                                           "fused_stacked16_layer_kernel<")), name
    finish = [n for n in kernels if "fused_layer_bwd16" in n and n not in mine]
    assert finish == ["whvi::fused_layer_bwd16_finish_kernel"], finish
    # the case list reaches exactly the shipped symbols
    assert tb.reached() == set(mine) | set(finish)
    # the pinned sets of the siblings, as tests/test_fastfood_stacked_bwd16_host.py restates them
    golden = [g for g in open(os.path.join(ROOT, "tests", "golden", "fused_shs_kernel_symbols_f32_f64.txt")).read().split("\n")
              if g.strip()]
    assert sorted(n for n in kernels if re.match(r"whvi::fused_shs_kernel<(float|double), ", n)) == sorted(golden)
    k_of = {"float": (4, 4, 4, 4, 4, 8, 16), "__half": (2, 2, 2, 2, 2, 4, 8), "__hip_bfloat16": (2, 2, 2, 2, 2, 4, 8)}
    bwd = {f"whvi::fused_shs_bwd_kernel<{t}, {L}, {ks[L - 6]}, {nt}>" for t, ks in k_of.items() for L in range(6, 13)
           for nt in ("true", "false")}
    assert {n for n in kernels if n.startswith("whvi::fused_shs_bwd_kernel<")} == bwd
    fwd = {f"whvi::fused_shs_stacked_kernel<float, {L}, {8 if L == 11 else 4}, {nt}>" for L in range(6, 12) for nt in ("true", "false")}
    assert {n for n in kernels if n.startswith("whvi::fused_shs_stacked_kernel<")} == fwd
    sbwd = {f"whvi::fused_shs_stacked_bwd_kernel<float, {L}, {8 if L == 11 else 4}, {J}, {nt}>"
            for L in range(6, 12) for J in range(2, 5) if _rule(L, J, 0) for nt in ("true", "false")}
    assert {n for n in kernels if n.startswith("whvi::fused_shs_stacked_bwd_kernel<")} == sbwd
    lbwd = {f"whvi::fused_shs_stacked_layer_bwd_kernel<float, {L}, {8 if L == 11 else 4}, {J}, {bias}, {nt}>"
            for L in range(6, 12) for J in range(2, 5) if _rule(L, J, 0) for bias in ("false", "true") for nt in ("true", "false")}
    assert {n for n in kernels if n.startswith("whvi::fused_shs_stacked_layer_bwd_kernel<")} == lbwd and len(lbwd) == 64
    assert len([n for n in kernels if "fused_shs_stacked_layer_bwd_finish_kernel" in n]) == 1
    lfwd = {f"whvi::fused_shs_stacked_layer_kernel<float, {L}, {8 if L == 11 else 4}, {nt}>" for L in range(6, 12) for nt in ("true", "false")}
    assert {n for n in kernels if n.startswith("whvi::fused_shs_stacked_layer_kernel<")} == lfwd
    b16 = {f"whvi::fused_stacked_bwd16_kernel<{t}, {L}, {K16[L]}, {J}, {nt}>"
           for t in TYPES for L in range(6, 12) for J in range(2, 5) if _rule(L, J, 0) for nt in ("true", "false")}
    assert {n for n in kernels if n.startswith("whvi::fused_stacked_bwd16_kernel<")} == b16 and len(b16) == 64
    assert [n for n in kernels if "stacked_bwd16" in n and n not in b16] == ["whvi::fused_stacked_bwd16_finish_kernel"]
    f16 = {f"whvi::fused_stacked16_kernel<{t}, {L}, {K16[L]}, {nt}>" for t in TYPES for L in range(6, 12) for nt in ("true", "false")}
    assert {n for n in kernels if "fused_stacked16_kernel<" in n} == f16
    l16 = {f"whvi::fused_stacked16_layer_kernel<{t}, {L}, {K16[L]}, {nt}>" for t in TYPES for L in range(6, 12)
           for nt in ("true", "false")}
    assert {n for n in kernels if "fused_stacked16_layer_kernel<" in n} == l16


def test_case_list():
    import slab_table as st
    import layer_bwd16_table as tb
    assert len(tb.CASES) == 128 and len({c["id"] for c in tb.CASES}) == 128
    seen = {}
    for c in tb.CASES:
        L, J, S, B = c["log2d"], c["J"], c["S"], c["B"]
        D = 1 << L
        la = tb.launch(c)
        assert S == 3 and _rule(L, J, c["bias"]) and st.ragged(S, B, L), c
        assert la.tiles_per_wave == st.tiles_per_wave(S, B, L) and la.grid == S * st.fused_bwd_geom(S, B, L)[0]
        assert la.symbols == (la.symbol, "whvi::fused_layer_bwd16_finish_kernel")
        assert la.symbol.endswith(f"{J}, {'true' if c['bias'] else 'false'}, {'true' if la.nt else 'false'}>")
        assert c["n_cols"] % 8 == 0 and c["ld"] % 8 == 0 and (J - 1) * D < c["n_cols"] <= J * D and c["ld"] >= c["n_cols"]
        assert (c["n_cols"] < J * D) == c["narrowed"] and (c["ld"] > c["n_cols"]) == c["wider"]
        if c["regime"] == "walk":
            assert not la.nt and la.tiles_per_wave >= 3 and tb.streamed_bytes(c) <= st.NT_MIN_BYTES, c
        else:
            assert la.nt and la.tiles_per_wave >= 2 and st.NT_MIN_BYTES < tb.streamed_bytes(c) < 1.5 * st.NT_MIN_BYTES, c
        seen.setdefault((c["dtype"], L, J, c["bias"]), set()).add(c["regime"])
        for opt in tb.OPTIONS:
            seen.setdefault((c["regime"], opt), set()).add(c[opt])
    for t in TYPES:
        for L, J in tb.SHIPPED_LJ:
            for bias in (False, True):
                assert seen[(t, L, J, bias)] == {"walk", "stream"}, (t, L, J, bias)
    for regime in ("walk", "stream"):
        for opt in tb.OPTIONS:
            assert seen[(regime, opt)] == {False, True}, (regime, opt)


# ---- the Module on host tensors: the composed route with the new flag off and on ---------------------------------------------
def _pass(layer, x, S, relu_in, relu_out, flag):
    sub = layer.weight_submodule
    sub.keep_half = sub.fused_epilogue = sub.fused_epilogue16 = sub.fused_backward = sub.fused_backward16 = True
    sub.fused_epilogue_backward16 = flag
    x = x.clone().requires_grad_()
    layer.zero_grad()
    torch.manual_seed(21)
    y = layer.forward_mc(x, S, relu_in=relu_in, relu_out=relu_out)
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(22)).to(y.dtype)
    (y * w).sum().backward()
    return y.detach(), x.grad, [p.grad.clone() for p in layer.parameters()]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n_in,n_out", [(16, 40), (10, 16)])
def test_the_flag_changes_nothing_on_host_tensors(n_in, n_out, dtype, monkeypatch):
    from whvi_amd import _hip
    S, B = 3, 5

    def no_launch(*args, **kwargs):
        raise AssertionError("a launch was called for host tensors")

    for name in ("fused_shs_stacked_layer_bwd16", "fused_shs_stacked_bwd16", "fused_shs_stacked_layer16"):
        monkeypatch.setattr(_hip, name, no_launch)
    layer = make_layer(n_in, n_out, bias=True)
    assert type(layer.weight_submodule).fused_epilogue_backward16 is False
    gen = torch.Generator().manual_seed(9)
    before = _hip.last_kernel()
    for x in (torch.randn(B, n_in, generator=gen).to(dtype), torch.randn(S, B, n_in, generator=gen).to(dtype)):
        for relu_in in (False, True):
            for relu_out in (False, True):
                y0, gx0, gp0 = _pass(layer, x, S, relu_in, relu_out, False)
                y1, gx1, gp1 = _pass(layer, x, S, relu_in, relu_out, True)
                assert y0.shape == (S, B, n_out) and y0.dtype == y1.dtype
                assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
                assert len(gp0) == len(gp1) == 4 * layer.weight_submodule.stack + 1
                for p, q in zip(gp0, gp1):
                    assert torch.equal(p, q)
    assert _hip.last_kernel() == before                                     # (no launch was named by any of these passes)


def test_the_function_keeps_its_thirteen_argument_call():
    import inspect
    from whvi_amd.fastfood import FastfoodStackedLayer16Function
    params = list(inspect.signature(FastfoodStackedLayer16Function.forward).parameters.values())
    assert [p.name for p in params[-3:]] == ["fused_backward", "fused_backward16", "fused_epilogue_backward16"]
    assert params[-1].default is False and len(params) == 1 + 14               # ctx + 13 + the new trailing flag


def test_routing_condition_from_the_measurements():
    """four blocks with the bias sum, or D = 2048, on more than 256 blocks of cached bytes stay composed."""
    from whvi_amd.fastfood import _layer_bwd16_pays as pays
    # (d, n_blocks, n_samples, sample_stride, n_cols, relu_out, shared, need_x, need_bias)
    assert pays(128, 4, 3, 65, 512, True, False, True, True)               # 9 blocks
    assert pays(128, 4, 16, 256, 512, True, False, True, True)             # 128 blocks
    assert not pays(128, 4, 64, 250, 512, True, False, True, True)         # 512 blocks, 41 MB
    assert not pays(128, 4, 64, 1000, 512, True, False, True, True)        # 1024 blocks, 164 MB: the measured row
    assert pays(128, 4, 64, 4000, 512, True, False, True, True)            # 655 MB: streams
    assert pays(128, 4, 64, 1000, 512, True, False, True, False)           # no bias sum
    assert pays(128, 3, 64, 1000, 384, True, False, True, True) and pays(128, 2, 64, 1000, 256, True, False, True, True)
    assert not pays(1024, 4, 64, 128, 4096, True, False, True, True) and pays(1024, 4, 16, 8192, 4096, True, False, True, True)
    assert pays(1024, 4, 3, 65, 4096, True, False, True, True)             # 51 blocks
    assert not pays(2048, 2, 64, 64, 4096, True, False, True, False) and pays(2048, 2, 16, 4096, 4096, True, False, True, True)
    assert pays(256, 4, 16, 8192, 800, True, False, True, True)            # 553 MB: streams
