"""The one-launch predictive pass of fastfood networks (whvi_mlp_fastfood_apply_f32, whvi_amd/fused_fastfood.py) without a
GPU: the C ABI is declared and exported, its supported rule is mirrored in Python, its argument checks answer before any HIP
call, the structural match takes fastfood networks and names its reasons for everything else (fused_mlp keeps refusing
them), the shipped library holds exactly the instantiations the dispatch reaches, without scratch, and on host tensors the
opt-in changes nothing."""
import ctypes
import itertools
import os
import re
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = {"relu": nn.ReLU, "sigmoid": nn.Sigmoid, "tanh": nn.Tanh}


def _net(n_in, D, n_mid=1, bias=True, bits=None, act="relu", modes=None):
    from whvi_amd.layers import WHVILinear
    from whvi_amd.networks import WHVIRegression
    bits = (1 << (n_mid + 1)) - 1 if bits is None else bits
    modes = modes or ["fastfood"] * n_mid
    mods = [WHVILinear(n_in, D, bias=bias)]
    for j in range(n_mid):
        mods += [ACTS[act]()] if (bits >> j) & 1 else []
        mods.append(WHVILinear(D, D, bias=bias, mode=modes[j]))
    mods += [ACTS[act]()] if (bits >> n_mid) & 1 else []
    mods.append(WHVILinear(D, 1, bias=bias))
    return WHVIRegression(mods)


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "whvi_hip.h")).read()
    assert "int whvi_mlp_fastfood_apply_supported(int32_t first, int32_t n_mid, int32_t log2d);" in header
    assert re.search(r"int whvi_mlp_fastfood_apply_f32\(void \*y, const void \*x, int32_t first, const void \*w_in, "
                     r"const void \*b_in, int32_t n_mid,\s+const void \*s1, const void \*s2, const void \*g, const void \*b_mid, "
                     r"int32_t mid_bias,\s+const void \*w_out, const void \*b_out, int64_t S, int64_t B, int32_t log2d, "
                     r"int32_t act,\s+int32_t act_bits, void \*stream\);", header)
    from whvi_amd import _hip
    L = _hip.lib()
    assert hasattr(L, "whvi_mlp_fastfood_apply_f32") and hasattr(L, "whvi_mlp_fastfood_apply_supported")
    assert L.whvi_hip_abi_version() == 1


def test_supported_rule_is_mirrored_in_python():
    from whvi_amd import _hip
    L = _hip.lib()
    for first in (0, 1, 2, 4, 8, 16):
        for n_mid in range(0, 6):
            for log2d in range(4, 13):
                want = bool(L.whvi_mlp_fastfood_apply_supported(first, n_mid, log2d))
                assert _hip.mlp_fastfood_apply_supported(first, n_mid, 1 << log2d) == want, (first, n_mid, log2d)
    # config 4 and the toy network fit; D = 2048 needs a column first layer and one square layer
    assert _hip.mlp_fastfood_apply_supported(4, 1, 1024) and _hip.mlp_fastfood_apply_supported(1, 1, 128)
    assert _hip.mlp_fastfood_apply_supported(1, 1, 2048) and not _hip.mlp_fastfood_apply_supported(4, 1, 2048)
    assert not _hip.mlp_fastfood_apply_supported(1, 2, 2048) and not _hip.mlp_fastfood_apply_supported(8, 2, 1024)
    assert _hip.mlp_fastfood_apply_supported(8, 4, 512) and not _hip.mlp_fastfood_apply_supported(4, 1, 4096)


def test_argument_checks_without_gpu():
    from whvi_amd import _hip
    L = _hip.lib()
    buf = (ctypes.c_char * 65536)()
    p = (ctypes.addressof(buf) + 15) & ~15
    x, w, s1, s2, g, wo, y = (p + 4096 * i for i in range(7))
    f = L.whvi_mlp_fastfood_apply_f32

    def call(y=y, x=x, first=4, w_in=w, b_in=None, n_mid=1, s1=s1, s2=s2, g=g, b_mid=None, mid_bias=0, w_out=wo, b_out=None,
             S=2, B=3, log2d=6, act=1, act_bits=3):
        return f(y, x, first, w_in, b_in, n_mid, s1, s2, g, b_mid, mid_bias, w_out, b_out, S, B, log2d, act, act_bits, None)

    for bad in (0, 4, -1):
        assert call(act=bad) == -1 and "act" in _hip.last_error(), bad
    assert call(act=0, S=0) == -1                                      # before "nothing to do"
    for act in (1, 2, 3):
        assert call(act=act, S=0) == 0 and _hip.last_error() == ""
        assert call(act=act, act_bits=4) == -1 and "act_bits" in _hip.last_error()
        assert call(act=act, S=-1) == -1 and "negative" in _hip.last_error()
        assert call(act=act, first=2) == -1 and "first-layer kind" in _hip.last_error()
        assert call(act=act, n_mid=5) == -2 and call(act=act, n_mid=0) == -2
        assert call(act=act, log2d=12) == -2 and call(act=act, log2d=5) == -2
        assert call(act=act, first=4, log2d=11) == -2 and "LDS" in _hip.last_error()
        assert call(act=act, first=1, n_mid=2, log2d=11) == -2 and "LDS" in _hip.last_error()
        assert call(act=act, mid_bias=2) == -1 and "mid_bias" in _hip.last_error()
        assert call(act=act, mid_bias=1) == -1 and "null" in _hip.last_error()     # b_mid needed
        for name in ("y", "x", "w_in", "s1", "s2", "g", "w_out"):
            assert call(act=act, **{name: None}) == -1 and "null" in _hip.last_error(), (act, name)
        for name, ptr in (("y", y), ("x", x), ("w_in", w), ("s1", s1), ("s2", s2), ("g", g), ("w_out", wo)):
            assert call(act=act, **{name: ptr + 4}) == -3, (act, name)
        assert call(act=act, b_out=p + 4) == -3 and "aligned" in _hip.last_error()
        assert call(act=act, y=g + 16) == -5 and "overlaps" in _hip.last_error()
    assert _hip.last_kernel() == "" or not _hip.last_kernel().startswith("whvi::mlp_fastfood_apply_kernel")


def test_match_takes_fastfood_networks():
    from whvi_amd import _hip, fused_fastfood
    for act in ACTS:
        for n_in, kind in ((1, _hip.MLP_FIRST_COLUMN), (3, _hip.MLP_FIRST_K4), (6, _hip.MLP_FIRST_K8)):
            for n_mid in (1, 2, 3, 4):
                for bits in range(1 << (n_mid + 1)):
                    p = fused_fastfood.match(_net(n_in, 64, n_mid, bits=bits, act=act))
                    assert isinstance(p, fused_fastfood.Plan), (act, n_in, n_mid, bits, p)
                    assert p.kind == kind and len(p.mids) == n_mid and p.D == 64 and p.act_bits == bits
                    assert p.act == (act if bits else "relu")
    p = fused_fastfood.match(_net(3, 1024))                         # config 4
    assert isinstance(p, fused_fastfood.Plan) and (p.kind, p.D, p.act, p.act_bits) == (4, 1024, "relu", 3)
    p = fused_fastfood.match(_net(1, 128, act="sigmoid"))           # the toy network
    assert isinstance(p, fused_fastfood.Plan) and (p.kind, p.D, p.act) == (1, 128, "sigmoid")
    assert isinstance(fused_fastfood.match(_net(1, 2048)), fused_fastfood.Plan)


def test_match_refuses_with_reasons():
    from whvi_amd import fused_fastfood, fused_mlp
    from whvi_amd.activations import Cosine
    from whvi_amd.layers import WHVILinear
    from whvi_amd.networks import WHVIRegression
    for modes in (["fastfood", "reference"], ["reference", "fastfood"]):
        reason = fused_fastfood.match(_net(3, 64, n_mid=2, modes=modes))
        assert isinstance(reason, str) and "mixed" in reason and "WHVISquarePow2Matrix" in reason, reason
    assert "no fastfood" in fused_fastfood.match(_net(3, 64, modes=["reference"]))
    for (na, a), (nb, b) in itertools.permutations({"ReLU": nn.ReLU, "Sigmoid": nn.Sigmoid, "Tanh": nn.Tanh}.items(), 2):
        net = WHVIRegression([WHVILinear(3, 64), a(), WHVILinear(64, 64, mode="fastfood"), b(), WHVILinear(64, 1)])
        reason = fused_fastfood.match(net)
        assert isinstance(reason, str) and na in reason and nb in reason, reason
    net = WHVIRegression([WHVILinear(3, 64), Cosine(), WHVILinear(64, 64, mode="fastfood"), WHVILinear(64, 1)])
    assert "Cosine" in fused_fastfood.match(net)
    for net, word in ((_net(3, 2048), "range"), (_net(1, 2048, n_mid=2), "range"), (_net(8, 1024, n_mid=2), "range"),
                      (_net(3, 4096), "range"), (_net(3, 64, n_mid=5), "at most 4"), (_net(12, 64), "K = 16")):
        reason = fused_fastfood.match(net)
        assert isinstance(reason, str) and word in reason, (word, reason)
    out2 = WHVIRegression([WHVILinear(3, 64), WHVILinear(64, 64, mode="fastfood"), WHVILinear(64, 2)])
    assert "one output" in fused_fastfood.match(out2)
    # fused_mlp keeps refusing fastfood networks with its own reason (tests/test_mlp_apply_host.py pins it)
    for net in (_net(3, 128), _net(1, 128, act="sigmoid"), _net(3, 64, n_mid=2, modes=["reference", "fastfood"])):
        reason = fused_mlp.match(net)
        assert isinstance(reason, str) and "WHVIFastfoodMatrix (mode='fastfood'?) is not a reference-mode WHVI matrix" in reason


def test_plan_needs_a_gpu_input():
    from whvi_amd import fused_fastfood
    net = _net(3, 128)
    with torch.no_grad():
        assert "CUDA" in fused_fastfood.plan(net, torch.randn(5, 3), 4)


def test_fastfood_mc_operands_are_forward_mc_draws():
    from whvi_amd.fastfood import WHVIFastfoodMatrix
    torch.manual_seed(0)
    w = WHVIFastfoodMatrix(64, bias=True)
    with torch.no_grad():
        w.g_mu.normal_()
        w.s1.normal_()
    torch.manual_seed(5)
    g = w._mc_operands(3)
    torch.manual_seed(5)
    eps = torch.randn(3, 64)
    assert torch.equal(g, w.g_mu + w.g_sigma * eps)
    x = torch.randn(3, 7, 64)
    torch.manual_seed(5)
    got = w.forward_mc(x, 3)
    import fwht_cpp
    H = lambda t: fwht_cpp.forward(t.reshape(-1, 64)).reshape(t.shape)   # noqa: E731
    want = w.s1 * H(g.unsqueeze(1) * H(w.s2 * x)) + w.bias
    assert torch.equal(got.detach(), want.detach())


# the dispatch of whvi_mlp_fastfood_apply_f32 (mlp_fastfood_apply.hip), restated
def _reached():
    from whvi_amd import _hip
    return {f"whvi::mlp_fastfood_apply_kernel<float, {log2d}, {kin}, {act}>"
            for log2d in range(6, 12) for kin in (1, 4, 8) for act in (1, 2, 3)
            if any(_hip.mlp_fastfood_apply_supported(kin, n, 1 << log2d) for n in range(1, 5))}


def test_shipped_library_holds_the_fastfood_kernels_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from shipped_isa import ShippedLibrary
    with ShippedLibrary() as lib:
        names = {n for n in lib.kernels if n.startswith("whvi::mlp_fastfood_apply_kernel<")}
        assert names == _reached() and len(names) == 48
        for name in names:
            k = lib.find(name)
            assert k["scratch"] == 0, name
            assert k["vgprs"] + k["agprs"] <= 256, (name, k["vgprs"], k["agprs"])      # two waves per SIMD or more


def test_flag_changes_nothing_on_host_tensors():
    for act, n_in in (("relu", 3), ("sigmoid", 1)):
        torch.manual_seed(0)
        net = _net(n_in, 64, act=act)
        net.eval_samples = 3
        x = torch.randn(7, n_in)
        net.eval()
        torch.manual_seed(1)
        want = net(x)
        net.set_fused_inference(True)
        torch.manual_seed(1)
        assert torch.equal(net(x), want)
