"""The trainable one-launch pass (whvi_mlp_apply_bwd_f32, fused_mlp.MLPApplyFunction, WHVINetwork.set_fused_training) without a
GPU: the C ABI is declared and exported, its range rule is mirrored in Python, its argument checks answer before any HIP call,
the shipped backward kernels use no scratch, the training plan names its reasons, and on host tensors the flag changes nothing."""
import ctypes
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_mlp_apply_host import _net  # noqa: E402


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "whvi_hip.h")).read()
    assert re.search(r"int whvi_mlp_apply_bwd_f32\(void \*grad_w_in, void \*grad_w_mid, void \*grad_w_out, void \*grad_b,", header)
    assert "int whvi_mlp_apply_bwd_supported(int32_t first, int32_t n_mid, int32_t log2d);" in header
    assert "int64_t whvi_mlp_apply_bwd_workspace(int64_t S, int64_t B, int32_t first, int32_t n_mid, int32_t log2d);" in header
    from whvi_amd import _hip
    L = _hip.lib()
    for name in ("whvi_mlp_apply_bwd_f32", "whvi_mlp_apply_bwd_supported", "whvi_mlp_apply_bwd_workspace"):
        assert hasattr(L, name), name
    assert L.whvi_hip_abi_version() == 1


def test_supported_rule_is_mirrored_in_python():
    from whvi_amd import _hip
    L = _hip.lib()
    for first in (0, 1, 2, 4, 8, 16):
        for n_mid in range(0, 6):
            for log2d in range(4, 13):
                want = bool(L.whvi_mlp_apply_bwd_supported(first, n_mid, log2d))
                assert _hip.mlp_apply_bwd_supported(first, n_mid, 1 << log2d) == want, (first, n_mid, log2d)
                if want:
                    assert _hip.mlp_apply_supported(first, n_mid, 1 << log2d)
                    assert L.whvi_mlp_apply_bwd_workspace(3, 100, first, n_mid, log2d) > 0
                else:
                    assert L.whvi_mlp_apply_bwd_workspace(3, 100, first, n_mid, log2d) == -1
    # the range the reference's networks need: toy / UCI (D = 128), config 4 (D = 1024), and K in {1, 4} everywhere
    for first in (1, 4, 8):
        assert _hip.mlp_apply_bwd_supported(first, 1, 128)
    assert _hip.mlp_apply_bwd_supported(4, 1, 1024) and _hip.mlp_apply_bwd_supported(8, 1, 1024)
    for d in (64, 128, 256, 512, 1024):
        for n_mid in (1, 2):
            for first in (1, 4):
                assert _hip.mlp_apply_bwd_supported(first, n_mid, d), (first, n_mid, d)
    assert not _hip.mlp_apply_bwd_supported(4, 3, 128) and not _hip.mlp_apply_bwd_supported(4, 1, 2048)


def test_argument_checks_without_gpu():
    from whvi_amd import _hip
    L = _hip.lib()
    buf = (ctypes.c_char * 65536)()
    p = (ctypes.addressof(buf) + 15) & ~15
    gwi, gwm, gwo, gb, work, g, x, w, s1, s2, u, wo = (p + 4096 * i for i in range(12))
    f = L.whvi_mlp_apply_bwd_f32
    need = L.whvi_mlp_apply_bwd_workspace(2, 3, 4, 1, 6)
    assert need > 0

    def call(grad_w_in=gwi, grad_w_mid=gwm, grad_w_out=gwo, grad_b=gb, grad_x=None, work=work, work_floats=need, g=g, x=x,
             first=4, w_in=w, b_in=None, n_mid=1, s1=s1, s2=s2, u=u, b_mid=None, mid_bias=0, w_out=wo, S=2, B=3, log2d=6, relu=3):
        return f(grad_w_in, grad_w_mid, grad_w_out, grad_b, grad_x, work, work_floats, g, x, first, w_in, b_in, n_mid, s1, s2, u,
                 b_mid, mid_bias, w_out, S, B, log2d, relu, None)

    assert call(S=-1) == -1 and "negative" in _hip.last_error()
    assert call(B=-1) == -1
    assert call(first=2) == -1 and "first-layer kind" in _hip.last_error()
    assert call(first=16) == -1
    for bad in (dict(n_mid=0), dict(n_mid=3), dict(log2d=5), dict(log2d=11), dict(first=8, log2d=11)):
        assert call(**bad) == -2 and "unsupported" in _hip.last_error(), bad
    assert call(relu=4) == -1 and "relu" in _hip.last_error()
    assert call(mid_bias=2) == -1 and "mid_bias" in _hip.last_error()
    assert call(S=0) == 0 and _hip.last_error() == ""
    assert call(S=1 << 16, B=1 << 16) == -2 and "32 bits" in _hip.last_error()
    for name in ("grad_w_in", "grad_w_mid", "grad_w_out", "grad_b", "work", "g", "x", "w_in", "s1", "s2", "u", "w_out"):
        assert call(**{name: None}) == -1 and "null" in _hip.last_error(), name
    assert call(mid_bias=1, b_mid=None) == -1 and "null" in _hip.last_error()
    for name, ptr in (("grad_w_in", gwi), ("work", work), ("x", x), ("w_in", w), ("s1", s1), ("u", u), ("w_out", wo)):
        assert call(**{name: ptr + 4}) == -3, name
    assert call(grad_x=p + 4) == -3 and "aligned" in _hip.last_error()
    assert call(work_floats=need - 1) == -1 and "workspace" in _hip.last_error()
    assert call(work_floats=0) == -1


def test_shipped_library_holds_the_backward_kernels_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from shipped_isa import ShippedLibrary
    from whvi_amd import _hip
    with ShippedLibrary() as lib:
        found = {n: k for n, k in lib.kernels.items() if n.startswith("whvi::mlp_apply_bwd_kernel<")}
        count = 0
        for log2d in range(6, 12):
            for kin in (1, 4, 8):
                for n_mid in (1, 2, 3, 4):
                    name = f"whvi::mlp_apply_bwd_kernel<float, {log2d}, {kin}, {n_mid}>"
                    if not _hip.mlp_apply_bwd_supported(kin, n_mid, 1 << log2d):
                        assert name not in found, name
                        continue
                    k = lib.find(name)
                    count += 1
                    assert k["scratch"] == 0, name
                    # register budget: two waves per SIMD (<= 256 per lane) wherever the accumulators -- 4 C (K + 2 + 2 n_mid)
                    # floats per lane -- allow it, config 4's K = 4 / one square layer at D = 1024 included; K = 8 with two
                    # square layers, or K = 8 or two square layers at D >= 512: one wave, and no spill to scratch
                    one_wave = (kin == 8 and n_mid == 2) or (log2d >= 9 and (kin == 8 or n_mid == 2))
                    budget = 512 if one_wave else 256
                    assert k["vgprs"] + k["agprs"] <= budget, (name, k["vgprs"], k["agprs"])
        assert count == len(found) == 30
        fin = lib.find("whvi::mlp_apply_bwd_finish_kernel")
        assert fin["scratch"] == 0


def test_training_plan_accepts_the_canonical_networks_and_names_reasons():
    from whvi_amd import _hip, fused_mlp
    # structural part (host tensors: the plan stops at the device check, the range check is the mirror)
    for args, n_mid in (((3, 1024), 1), ((6, 128), 1), ((1, 128), 1), ((8, 256, 2), 2), ((4, 64), 1), ((1, 512, 2), 2)):
        p = fused_mlp.match(_net(*args))
        assert isinstance(p, fused_mlp.Plan), args
        assert _hip.mlp_apply_bwd_supported(p.kind, len(p.mids), p.D), args
    for args in ((5, 512, 4), (3, 2048), (3, 64, 3)):
        p = fused_mlp.match(_net(*args))
        assert isinstance(p, fused_mlp.Plan) and not _hip.mlp_apply_bwd_supported(p.kind, len(p.mids), p.D), args
    net = _net(3, 128)
    reason = fused_mlp.plan(net, torch.randn(5, 3), 4, training=True)
    assert isinstance(reason, str) and "CUDA" in reason
    assert "K = 2" in fused_mlp.plan(_net(2, 128), torch.randn(5, 2), 4, training=True)
    # the predictive plan keeps its answers
    with torch.no_grad():
        assert "CUDA" in fused_mlp.plan(net, torch.randn(5, 3), 4)
    assert isinstance(fused_mlp.match(net), fused_mlp.Plan)


def test_flag_changes_nothing_on_host_tensors():
    for args in ((3, 64), (1, 64)):
        for mode in ("auto", "batched"):
            torch.manual_seed(0)
            net = _net(*args, train_samples=3).train()
            net.mc_mode = mode
            x, y = torch.randn(7, args[0]), torch.randn(7, 1)
            results = []
            for on in (False, True):
                net.set_fused_training(on)
                assert net.fused_training is on
                net.zero_grad(set_to_none=True)
                torch.manual_seed(1)
                loss = net.loss(x, y, n=7)
                loss.backward()
                results.append((loss.detach().clone(), [p.grad.clone() for p in net.parameters() if p.grad is not None]))
            (l0, g0), (l1, g1) = results
            assert torch.equal(l0, l1), (args, mode)
            assert len(g0) == len(g1) > 0 and all(torch.equal(a, b) for a, b in zip(g0, g1)), (args, mode)
    assert _net(3, 64).fused_training is False
    assert _net(3, 64).set_fused_training().fused_training is True and _net(3, 64).set_fused_training().fused_inference is False
