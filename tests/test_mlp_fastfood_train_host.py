"""The trainable one-launch pass of fastfood networks (whvi_mlp_fastfood_apply_bwd_f32, fused_fastfood.FastfoodMLPApplyFunction,
WHVINetwork.set_fused_training) without a GPU: the C ABI is declared and exported, its supported rule and workspace are
mirrored in Python, every argument check answers before any HIP call, the training plan names its reasons (the predictive
plan's stay word for word), the shipped library holds exactly the instantiations the dispatch reaches, without scratch, and on
host tensors the opt-in changes nothing."""
import ctypes
import os
import re
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = {"relu": nn.ReLU, "sigmoid": nn.Sigmoid, "tanh": nn.Tanh}


def _net(n_in, D, n_mid=1, bias=True, act="relu", modes=None):
    from whvi_amd.layers import WHVILinear
    from whvi_amd.networks import WHVIRegression
    modes = modes or ["fastfood"] * n_mid
    mods = [WHVILinear(n_in, D, bias=bias)]
    for j in range(n_mid):
        mods += [ACTS[act](), WHVILinear(D, D, bias=bias, mode=modes[j])]
    mods += [ACTS[act](), WHVILinear(D, 1, bias=bias)]
    return WHVIRegression(mods)


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "whvi_hip.h")).read()
    assert "int whvi_mlp_fastfood_apply_bwd_supported(int32_t first, int32_t n_mid, int32_t log2d);" in header
    assert ("int64_t whvi_mlp_fastfood_apply_bwd_workspace(int64_t S, int64_t B, int32_t first, int32_t n_mid, int32_t log2d);"
            in header)
    assert re.search(r"int whvi_mlp_fastfood_apply_bwd_f32\(void \*grad_w_in, void \*grad_s1, void \*grad_s2, void \*grad_g, "
                     r"void \*grad_w_out, void \*grad_b,\s+void \*grad_x, void \*work, int64_t work_floats, const void \*g, "
                     r"const void \*x, int32_t first,\s+const void \*w_in, const void \*b_in, int32_t n_mid, const void \*s1, "
                     r"const void \*s2,\s+const void \*gk, const void \*b_mid, int32_t mid_bias, const void \*w_out, int64_t S, "
                     r"int64_t B,\s+int32_t log2d, int32_t act, int32_t act_bits, void \*stream\);", header)
    from whvi_amd import _hip
    L = _hip.lib()
    for name in ("whvi_mlp_fastfood_apply_bwd_supported", "whvi_mlp_fastfood_apply_bwd_workspace", "whvi_mlp_fastfood_apply_bwd_f32"):
        assert hasattr(L, name), name
    assert L.whvi_hip_abi_version() == 1


def test_supported_rule_and_workspace_are_mirrored_in_python():
    from whvi_amd import _hip
    L = _hip.lib()
    for first in (1, 4, 8, 2):
        for n_mid in range(0, 6):
            for log2d in range(5, 13):
                want = bool(L.whvi_mlp_fastfood_apply_bwd_supported(first, n_mid, log2d))
                assert _hip.mlp_fastfood_apply_bwd_supported(first, n_mid, 1 << log2d) == want, (first, n_mid, log2d)
                assert want == (_hip.mlp_fastfood_apply_supported(first, n_mid, 1 << log2d) and n_mid <= 2 and log2d <= 10)
                ws = L.whvi_mlp_fastfood_apply_bwd_workspace(3, 700, first, n_mid, log2d)
                assert (ws == -1) == (not want), (first, n_mid, log2d, ws)
                if want:
                    part = ((first + 2 + 4 * n_mid) << log2d) + 4
                    assert ws > 0 and ws % (3 * part) == 0
                    assert L.whvi_mlp_fastfood_apply_bwd_workspace(0, 700, first, n_mid, log2d) == 0
                    assert L.whvi_mlp_fastfood_apply_bwd_workspace(3, 0, first, n_mid, log2d) == 0
                    assert L.whvi_mlp_fastfood_apply_bwd_workspace(-1, 5, first, n_mid, log2d) == -1
    # the shapes the range must keep: config 4, the toy and the UCI network with one and two layers, every K at D <= 512
    assert _hip.mlp_fastfood_apply_bwd_supported(4, 1, 1024)
    for n_mid in (1, 2):
        assert _hip.mlp_fastfood_apply_bwd_supported(1, n_mid, 128) and _hip.mlp_fastfood_apply_bwd_supported(8, n_mid, 128)
        for kin in (1, 4, 8):
            for d in (64, 128, 256, 512):
                assert _hip.mlp_fastfood_apply_bwd_supported(kin, n_mid, d)
    assert not _hip.mlp_fastfood_apply_bwd_supported(1, 1, 2048) and not _hip.mlp_fastfood_apply_bwd_supported(4, 3, 128)
    assert not _hip.mlp_fastfood_apply_bwd_supported(8, 2, 1024)


def test_argument_checks_without_gpu():
    from whvi_amd import _hip
    L = _hip.lib()
    buf = (ctypes.c_char * (1 << 20))()
    p = (ctypes.addressof(buf) + 15) & ~15
    step = 32768
    names = ("grad_w_in", "grad_s1", "grad_s2", "grad_g", "grad_w_out", "grad_b", "grad_x", "work", "g", "x", "w_in", "s1", "s2",
             "gk", "w_out")
    at = {n: p + step * i for i, n in enumerate(names)}
    f = L.whvi_mlp_fastfood_apply_bwd_f32
    need = L.whvi_mlp_fastfood_apply_bwd_workspace(2, 3, 4, 1, 6)
    assert 0 < need * 4 <= step

    def call(first=4, b_in=None, n_mid=1, b_mid=None, mid_bias=0, S=2, B=3, log2d=6, act=1, act_bits=3, work_floats=need, **kw):
        a = dict(at, **kw)
        return f(a["grad_w_in"], a["grad_s1"], a["grad_s2"], a["grad_g"], a["grad_w_out"], a["grad_b"], a["grad_x"], a["work"],
                 work_floats, a["g"], a["x"], first, a["w_in"], b_in, n_mid, a["s1"], a["s2"], a["gk"], b_mid, mid_bias,
                 a["w_out"], S, B, log2d, act, act_bits, None)

    for bad in (0, 4, -1):
        assert call(act=bad) == -1 and "act" in _hip.last_error(), bad
    assert call(act=0, S=0) == -1                                      # before "nothing to do"
    for act in (1, 2, 3):
        assert call(act=act, S=0) == 0 and _hip.last_error() == ""
        assert call(act=act, act_bits=4) == -1 and "act_bits" in _hip.last_error()
        assert call(act=act, S=-1) == -1 and "negative" in _hip.last_error()
        assert call(act=act, first=2) == -1 and "first-layer kind" in _hip.last_error()
        assert call(act=act, n_mid=3) == -2 and call(act=act, n_mid=0) == -2 and call(act=act, n_mid=5) == -2
        assert call(act=act, log2d=11, first=1) == -2 and call(act=act, log2d=5) == -2
        assert call(act=act, first=8, n_mid=2, log2d=10) == -2 and "unsupported" in _hip.last_error()
        assert call(act=act, mid_bias=2) == -1 and "mid_bias" in _hip.last_error()
        assert call(act=act, mid_bias=1) == -1 and "null" in _hip.last_error()     # b_mid needed
        assert call(act=act, S=1 << 20, B=1 << 12) == -2 and "32 bits" in _hip.last_error()
        for name in names:
            if name != "grad_x":                                           # grad_x is optional
                assert call(act=act, **{name: None}) == -1 and "null" in _hip.last_error(), (act, name)
        for name in names:
            assert call(act=act, **{name: at[name] + 4}) == -3 and "aligned" in _hip.last_error(), (act, name)
        assert call(act=act, b_in=p + 4) == -3
        assert call(act=act, work_floats=need - 1) == -1 and "workspace" in _hip.last_error()
        for out in ("grad_w_in", "grad_s1", "grad_s2", "grad_g", "grad_w_out", "grad_b", "grad_x", "work"):
            for src in ("g", "x", "w_in", "s1", "s2", "gk", "w_out"):
                assert call(act=act, **{out: at[src]}) == -5 and "overlaps" in _hip.last_error(), (out, src)
        assert call(act=act, grad_x=None, work=at["gk"] + 16) == -5
    assert "mlp_fastfood_apply_bwd" not in _hip.last_kernel()


def test_training_plan_reasons_on_host_tensors():
    from whvi_amd import fused_fastfood
    x = torch.randn(5, 3)
    net = _net(3, 128)
    assert "CUDA" in fused_fastfood.plan(net, x, 4, training=True)
    with torch.no_grad():
        assert "CUDA" in fused_fastfood.plan(net, x, 4)                 # the predictive plan's reasons, word for word
    assert fused_fastfood.plan(_net(3, 128, modes=["reference"]), x, 4, training=True) == \
        "no fastfood square layer (mode='fastfood'): the reference-mode networks are fused_mlp's"
    assert "range" in fused_fastfood.plan(_net(3, 4096), x, 4, training=True)
    # whole strings, from what plan() returns: a host input is refused first, a network outside the forward's range by match.
    # The reasons behind the device check (graph wanted / not wanted, the backward's range) are asserted with == on the GPU:
    # tests/test_fused_refusals_gpu.py
    for training in (True, False):
        with torch.set_grad_enabled(training):
            assert fused_fastfood.plan(net, x, 4, training=training) == "input: needs a float32 CUDA (batch, 3) tensor"
            assert fused_fastfood.plan(_net(3, 4096), x, 4, training=training) == \
                "hidden width 4096 with 1 fastfood layers is outside whvi_mlp_fastfood_apply's range"


# the dispatch of whvi_mlp_fastfood_apply_bwd_f32 (mlp_fastfood_apply_bwd.hpp), restated
def _reached():
    from whvi_amd import _hip
    return {f"whvi::mlp_fastfood_apply_bwd_kernel<float, {log2d}, {kin}, {n_mid}, {act}>"
            for log2d in range(6, 11) for kin in (1, 4, 8) for n_mid in (1, 2) for act in (1, 2, 3)
            if _hip.mlp_fastfood_apply_bwd_supported(kin, n_mid, 1 << log2d)}


def test_shipped_library_holds_the_backward_kernels_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from shipped_isa import ShippedLibrary
    with ShippedLibrary() as lib:
        names = {n for n in lib.kernels if n.startswith("whvi::mlp_fastfood_apply_bwd_kernel<")}
        assert names == _reached() and len(names) == 87
        for name in sorted(names) + ["whvi::mlp_fastfood_apply_bwd_finish_kernel"]:
            k = lib.find(name)
            assert k["scratch"] == 0, name
            assert k["vgprs"] + k["agprs"] <= 512, (name, k["vgprs"], k["agprs"])


def test_flag_changes_nothing_on_host_tensors():
    for act, n_in in (("relu", 3), ("sigmoid", 1)):
        torch.manual_seed(0)
        net = _net(n_in, 64, act=act).train()
        net.train_samples = 3
        x, y = torch.randn(7, n_in), torch.randn(7, 1)
        results = []
        for on in (False, True):
            net.set_fused_training(on)
            net.zero_grad(set_to_none=True)
            torch.manual_seed(1)
            loss = net.loss(x, y, n=7)
            loss.backward()
            results.append((loss.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters()}))
        assert torch.equal(results[0][0], results[1][0])
        for k in results[0][1]:
            assert torch.equal(results[0][1][k], results[1][1][k]), k
