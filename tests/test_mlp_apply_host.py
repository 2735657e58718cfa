"""The one-launch predictive pass (whvi_mlp_apply_f32, whvi_amd/fused_mlp.py) without a GPU: the C ABI is declared and
exported, its argument checks answer before any HIP call, the structural match accepts the canonical networks and names
its reason for everything else, the shipped kernels use no scratch, and on host tensors the opt-in changes nothing."""
import ctypes
import os
import re
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(n_in, D, n_mid=1, bias=True, relus=(True, True), act=nn.ReLU, out=1, mode="reference", **kw):
    from whvi_amd.layers import WHVILinear
    from whvi_amd.networks import WHVIRegression
    relus = list(relus) + [relus[-1]] * (n_mid + 1 - len(relus))
    mods = [WHVILinear(n_in, D, bias=bias)]
    for j in range(n_mid):
        if relus[j]:
            mods.append(act())
        mods.append(WHVILinear(D, D, bias=bias, mode=mode))
    if relus[n_mid]:
        mods.append(act())
    mods.append(WHVILinear(D, out, bias=bias))
    return WHVIRegression(mods, **kw)


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "whvi_hip.h")).read()
    assert re.search(r"int whvi_mlp_apply_f32\(void \*y, const void \*x, int32_t first,", header)
    assert "int whvi_mlp_apply_supported(int32_t first, int32_t n_mid, int32_t log2d);" in header
    for name in ("WHVI_MLP_FIRST_COLUMN 1", "WHVI_MLP_FIRST_K4     4", "WHVI_MLP_FIRST_K8     8"):
        assert "#define " + name in header
    from whvi_amd import _hip
    L = _hip.lib()
    assert hasattr(L, "whvi_mlp_apply_f32") and hasattr(L, "whvi_mlp_apply_supported")
    assert L.whvi_hip_abi_version() == 1


def test_supported_rule_is_mirrored_in_python():
    from whvi_amd import _hip
    L = _hip.lib()
    for first in (0, 1, 2, 4, 8, 16):
        for n_mid in range(0, 6):
            for log2d in range(4, 13):
                want = bool(L.whvi_mlp_apply_supported(first, n_mid, log2d))
                assert _hip.mlp_apply_supported(first, n_mid, 1 << log2d) == want, (first, n_mid, log2d)
    # the shapes the reference uses, and the edges of the LDS rule
    assert _hip.mlp_apply_supported(4, 1, 1024) and _hip.mlp_apply_supported(8, 1, 128) and _hip.mlp_apply_supported(1, 1, 128)
    assert _hip.mlp_apply_supported(8, 2, 256) and _hip.mlp_apply_supported(4, 4, 1024) and _hip.mlp_apply_supported(4, 1, 2048)
    assert not _hip.mlp_apply_supported(8, 1, 2048)            # 96 KiB of one sample's operands
    assert not _hip.mlp_apply_supported(4, 1, 4096) and not _hip.mlp_apply_supported(4, 1, 32)


def test_argument_checks_without_gpu():
    from whvi_amd import _hip
    L = _hip.lib()
    buf = (ctypes.c_char * 65536)()
    p = (ctypes.addressof(buf) + 15) & ~15
    x, w, s1, s2, u, wo, y = (p + 4096 * i for i in range(7))
    f = L.whvi_mlp_apply_f32

    def call(y=y, x=x, first=4, w_in=w, b_in=None, n_mid=1, s1=s1, s2=s2, u=u, b_mid=None, mid_bias=0, w_out=wo, b_out=None,
             S=2, B=3, log2d=6, relu=3):
        return f(y, x, first, w_in, b_in, n_mid, s1, s2, u, b_mid, mid_bias, w_out, b_out, S, B, log2d, relu, None)

    assert call(S=-1) == -1 and "negative" in _hip.last_error()
    assert call(B=-1) == -1
    assert call(first=2) == -1 and "first-layer kind" in _hip.last_error()
    assert call(first=16) == -1
    assert call(n_mid=0) == -2 and "n_mid" in _hip.last_error()
    assert call(n_mid=5) == -2
    assert call(log2d=5) == -2 and "log2(D)" in _hip.last_error()
    assert call(log2d=12) == -2
    assert call(first=8, log2d=11) == -2 and "LDS" in _hip.last_error()
    assert call(relu=4) == -1 and "relu" in _hip.last_error()           # n_mid = 1: two boundaries
    assert call(mid_bias=2) == -1 and "mid_bias" in _hip.last_error()
    assert call(S=0) == 0 and _hip.last_error() == ""                   # nothing to do
    assert call(B=0, y=None, x=None) == 0
    assert call(S=1 << 16, B=1 << 16) == -2 and "32 bits" in _hip.last_error()
    for name in ("y", "x", "w_in", "s1", "s2", "u", "w_out"):
        assert call(**{name: None}) == -1 and "null" in _hip.last_error(), name
    assert call(mid_bias=1, b_mid=None) == -1 and "null" in _hip.last_error()
    for name, ptr in (("y", y), ("x", x), ("w_in", w), ("s1", s1), ("s2", s2), ("u", u), ("w_out", wo)):
        assert call(**{name: ptr + 4}) == -3, name
    assert call(b_in=p + 4) == -3 and call(b_out=p + 4) == -3 and call(mid_bias=1, b_mid=p + 4) == -3
    assert "aligned" in _hip.last_error()
    assert call(y=x) == -5 and "overlaps" in _hip.last_error()          # y on top of x
    assert call(y=w + 16) == -5                                         # y inside w_in (S * D * K floats)
    assert call(b_out=y + 16) == -5
    assert call(b_in=y) == -5


def test_match_accepts_the_canonical_networks():
    from whvi_amd import _hip, fused_mlp
    cases = [((3, 1024), _hip.MLP_FIRST_K4, 1), ((6, 128), _hip.MLP_FIRST_K8, 1), ((1, 128), _hip.MLP_FIRST_COLUMN, 1),
             ((8, 256, 2), _hip.MLP_FIRST_K8, 2), ((4, 64), _hip.MLP_FIRST_K4, 1), ((5, 512, 4), _hip.MLP_FIRST_K8, 4)]
    for args, kind, n_mid in cases:
        for bias in (True, False):
            p = fused_mlp.match(_net(*args, bias=bias))
            assert isinstance(p, fused_mlp.Plan), (args, bias, p)
            assert p.kind == kind and len(p.mids) == n_mid and p.D == args[1] and p.n_in == args[0]
            assert p.relu == (1 << (n_mid + 1)) - 1
    # every combination of ReLUs at the two boundaries
    for relus, bits in (((True, True), 3), ((False, True), 2), ((True, False), 1), ((False, False), 0)):
        p = fused_mlp.match(_net(3, 1024, relus=relus))
        assert isinstance(p, fused_mlp.Plan) and p.relu == bits
    p = fused_mlp.match(_net(8, 256, n_mid=2, relus=(True, False, True)))
    assert p.relu == 0b101


def test_match_rejects_with_a_reason():
    from whvi_amd import fused_mlp
    from whvi_amd.activations import Cosine
    from whvi_amd.layers import WHVILinear
    from whvi_amd.networks import WHVIRegression
    rejected = {
        "K = 2": _net(2, 128),
        "K = 16": _net(9, 128),
        "cosine": _net(3, 128, act=Cosine),
        "fastfood": _net(3, 128, mode="fastfood"),
        "faithful": _net(3, 128).set_faithful_dataflow(True),
        "two outputs": _net(3, 128, out=2),
        "width 100": _net(3, 100),
        "width 96, column first": _net(1, 96),
        "five square layers": _net(3, 64, n_mid=5),
        "D = 4096": _net(3, 4096),
        "leading ReLU": WHVIRegression([nn.ReLU(), WHVILinear(3, 64), WHVILinear(64, 64), WHVILinear(64, 1)]),
        "trailing ReLU": WHVIRegression([WHVILinear(3, 64), WHVILinear(64, 64), WHVILinear(64, 1), nn.ReLU()]),
        "two ReLUs": WHVIRegression([WHVILinear(3, 64), nn.ReLU(), nn.ReLU(), WHVILinear(64, 64), WHVILinear(64, 1)]),
        "no square layer": WHVIRegression([WHVILinear(3, 64), nn.ReLU(), WHVILinear(64, 1)]),
    }
    for what, net in rejected.items():
        reason = fused_mlp.match(net)
        assert isinstance(reason, str) and reason, what
    assert "K = 2" in fused_mlp.match(rejected["K = 2"]) and "K = 16" in fused_mlp.match(rejected["K = 16"])
    assert "Cosine" in fused_mlp.match(rejected["cosine"])
    assert "fastfood" in fused_mlp.match(rejected["fastfood"])
    assert "faithful" in fused_mlp.match(rejected["faithful"])
    assert "one output" in fused_mlp.match(rejected["two outputs"])


def test_plan_needs_a_gpu_input():
    from whvi_amd import fused_mlp
    with torch.no_grad():
        assert "CUDA" in fused_mlp.plan(_net(3, 128), torch.randn(5, 3), 4)


def test_shipped_library_holds_the_kernels_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from shipped_isa import ShippedLibrary
    from whvi_amd import _hip
    with ShippedLibrary() as lib:
        found = {n: k for n, k in lib.kernels.items() if n.startswith("whvi::mlp_apply_kernel<")}
        for log2d in range(6, 12):
            for kin in (1, 4, 8):
                name = f"whvi::mlp_apply_kernel<float, {log2d}, {kin}>"
                if not any(_hip.mlp_apply_supported(kin, n, 1 << log2d) for n in range(1, 5)):
                    assert name not in found
                    continue
                k = lib.find(name)
                assert k["scratch"] == 0, name
                # register budget: at least two waves per SIMD up to D = 1024 (512 registers per lane and SIMD); D = 2048
                # holds 64 hidden floats and twice the operand chunks per lane -- one wave, but no spill to scratch
                budget = 256 if log2d <= 10 else 512
                assert k["vgprs"] + k["agprs"] <= budget, (name, k["vgprs"], k["agprs"])
        assert len(found) == 17


def test_flag_changes_nothing_on_host_tensors():
    for args in ((3, 64), (1, 64)):
        torch.manual_seed(0)
        net = _net(*args, eval_samples=3).eval()
        x = torch.randn(7, args[0])
        torch.manual_seed(1)
        want = net(x)
        net.set_fused_inference(True)
        assert net.fused_inference is True
        torch.manual_seed(1)
        assert torch.equal(net(x), want)
        net.mc_mode = "batched"                 # the batched route on the host: no plan (host tensors), same draws
        torch.manual_seed(2)
        got = net(x)
        net.set_fused_inference(False)
        torch.manual_seed(2)
        assert torch.equal(got, net(x))
    assert _net(3, 64).fused_inference is False
