"""Sigmoid and tanh in the one-launch passes (whvi_mlp_apply_act_f32, whvi_mlp_apply_act_bwd_f32, fused_mlp.match) without a
GPU: the C ABI is declared and exported, its argument checks answer before any HIP call, the structural match takes Sigmoid
and Tanh networks at every boundary combination and names its reasons for mixtures, the shipped library holds exactly the
smooth instantiations the dispatch reaches -- without scratch, inside the ReLU kernels' register budgets -- and on host
tensors the flags change nothing."""
import ctypes
import itertools
import os
import re
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_mlp_apply_host import _net  # noqa: E402

ACTS = {"sigmoid": (nn.Sigmoid, 2), "tanh": (nn.Tanh, 3)}


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "whvi_hip.h")).read()
    assert re.search(r"int whvi_mlp_apply_act_f32\(void \*y, const void \*x, int32_t first,", header)
    assert re.search(r"int whvi_mlp_apply_act_bwd_f32\(void \*grad_w_in, void \*grad_w_mid,", header)
    assert re.search(r"int32_t log2d, int32_t act,\s+int32_t act_bits, void \*stream\);", header)
    for name in ("WHVI_MLP_ACT_RELU    1", "WHVI_MLP_ACT_SIGMOID 2", "WHVI_MLP_ACT_TANH    3"):
        assert "#define " + name in header
    from whvi_amd import _hip
    L = _hip.lib()
    assert hasattr(L, "whvi_mlp_apply_act_f32") and hasattr(L, "whvi_mlp_apply_act_bwd_f32")
    assert L.whvi_hip_abi_version() == 1
    assert _hip.MLP_ACTS == {"relu": 1, "sigmoid": 2, "tanh": 3}


def _buffers(n):
    buf = (ctypes.c_char * 65536)()
    p = (ctypes.addressof(buf) + 15) & ~15
    return buf, p, [p + 4096 * i for i in range(n)]


def test_forward_argument_checks_without_gpu():
    from whvi_amd import _hip
    L = _hip.lib()
    buf, p, (x, w, s1, s2, u, wo, y) = _buffers(7)
    f = L.whvi_mlp_apply_act_f32

    def call(y=y, x=x, first=4, w_in=w, b_in=None, n_mid=1, s1=s1, s2=s2, u=u, b_mid=None, mid_bias=0, w_out=wo, b_out=None,
             S=2, B=3, log2d=6, act=2, act_bits=3):
        return f(y, x, first, w_in, b_in, n_mid, s1, s2, u, b_mid, mid_bias, w_out, b_out, S, B, log2d, act, act_bits, None)

    for bad in (0, 4, -1, 99):
        assert call(act=bad) == -1 and "act" in _hip.last_error(), bad
    assert call(act=0, S=0) == -1                                      # before "nothing to do"
    for act in (1, 2, 3):
        assert call(act=act, act_bits=4) == -1 and "bits" in _hip.last_error(), act     # n_mid = 1: two boundaries
        assert call(act=act, n_mid=2, act_bits=8) == -1
        assert call(act=act, S=0) == 0 and _hip.last_error() == ""
        assert call(act=act, S=-1) == -1 and "negative" in _hip.last_error()
        assert call(act=act, first=2) == -1 and "first-layer kind" in _hip.last_error()
        assert call(act=act, n_mid=5) == -2 and call(act=act, log2d=12) == -2
        assert call(act=act, first=8, log2d=11) == -2 and "LDS" in _hip.last_error()
        assert call(act=act, mid_bias=2) == -1 and "mid_bias" in _hip.last_error()
        for name in ("y", "x", "w_in", "s1", "s2", "u", "w_out"):
            assert call(act=act, **{name: None}) == -1 and "null" in _hip.last_error(), (act, name)
        for name, ptr in (("y", y), ("x", x), ("w_in", w), ("s1", s1), ("u", u), ("w_out", wo)):
            assert call(act=act, **{name: ptr + 4}) == -3, (act, name)
        assert call(act=act, b_out=p + 4) == -3 and "aligned" in _hip.last_error()
        assert call(act=act, y=x) == -5 and "overlaps" in _hip.last_error()


def test_backward_argument_checks_without_gpu():
    from whvi_amd import _hip
    L = _hip.lib()
    buf, p, (gwi, gwm, gwo, gb, work, g, x, w, s1, s2, u, wo) = _buffers(12)
    f = L.whvi_mlp_apply_act_bwd_f32
    need = L.whvi_mlp_apply_bwd_workspace(2, 3, 4, 1, 6)

    def call(grad_w_in=gwi, grad_w_mid=gwm, grad_w_out=gwo, grad_b=gb, grad_x=None, work=work, work_floats=need, g=g, x=x,
             first=4, w_in=w, b_in=None, n_mid=1, s1=s1, s2=s2, u=u, b_mid=None, mid_bias=0, w_out=wo, S=2, B=3, log2d=6, act=3,
             act_bits=3):
        return f(grad_w_in, grad_w_mid, grad_w_out, grad_b, grad_x, work, work_floats, g, x, first, w_in, b_in, n_mid, s1, s2, u,
                 b_mid, mid_bias, w_out, S, B, log2d, act, act_bits, None)

    for bad in (0, 4, -3):
        assert call(act=bad) == -1 and "act" in _hip.last_error(), bad
    for act in (1, 2, 3):
        assert call(act=act, act_bits=4) == -1 and "bits" in _hip.last_error(), act
        assert call(act=act, S=0) == 0 and _hip.last_error() == ""
        for bad in (dict(n_mid=3), dict(log2d=11), dict(first=8, log2d=11)):
            assert call(act=act, **bad) == -2 and "unsupported" in _hip.last_error(), (act, bad)
        for name in ("grad_w_in", "grad_w_mid", "grad_w_out", "grad_b", "work", "g", "x", "w_in", "s1", "s2", "u", "w_out"):
            assert call(act=act, **{name: None}) == -1 and "null" in _hip.last_error(), (act, name)
        for name, ptr in (("grad_w_in", gwi), ("work", work), ("x", x), ("w_in", w), ("u", u)):
            assert call(act=act, **{name: ptr + 4}) == -3, (act, name)
        assert call(act=act, grad_x=p + 4) == -3 and "aligned" in _hip.last_error()
        assert call(act=act, work_floats=need - 1) == -1 and "workspace" in _hip.last_error()


def _smooth_net(n_in, D, n_mid, bits, act_cls, bias=True):
    from whvi_amd.layers import WHVILinear
    from whvi_amd.networks import WHVIRegression
    mods = [WHVILinear(n_in, D, bias=bias)]
    for j in range(n_mid):
        mods += [act_cls()] if (bits >> j) & 1 else []
        mods.append(WHVILinear(D, D, bias=bias))
    mods += [act_cls()] if (bits >> n_mid) & 1 else []
    mods.append(WHVILinear(D, 1, bias=bias))
    return WHVIRegression(mods)


def test_match_takes_sigmoid_and_tanh_at_every_boundary_combination():
    from whvi_amd import _hip, fused_mlp
    for act, (cls, _) in ACTS.items():
        for n_in, kind in ((1, _hip.MLP_FIRST_COLUMN), (3, _hip.MLP_FIRST_K4), (6, _hip.MLP_FIRST_K8)):
            for n_mid in (1, 2, 3, 4):
                for bits in range(1 << (n_mid + 1)):
                    p = fused_mlp.match(_smooth_net(n_in, 64, n_mid, bits, cls))
                    assert isinstance(p, fused_mlp.Plan), (act, n_in, n_mid, bits, p)
                    assert p.kind == kind and len(p.mids) == n_mid and p.D == 64
                    if bits == 0:          # no activation module at all: the ReLU kernels with no ReLU
                        assert (p.act, p.act_bits, p.relu) == ("relu", 0, 0)
                    else:
                        assert (p.act, p.act_bits, p.relu) == (act, bits, 0), (act, n_mid, bits, p.act, p.act_bits)
    # the notebook's model, and ReLU networks keep their plan
    p = fused_mlp.match(_smooth_net(1, 128, 1, 3, nn.Sigmoid))
    assert (p.act, p.act_bits, p.relu, p.kind) == ("sigmoid", 3, 0, _hip.MLP_FIRST_COLUMN)
    p = fused_mlp.match(_net(8, 256, n_mid=2, relus=(True, False, True)))
    assert (p.act, p.act_bits, p.relu) == ("relu", 0b101, 0b101)


def test_match_rejects_mixtures_and_cosine_with_reasons():
    from whvi_amd import fused_mlp
    from whvi_amd.activations import Cosine
    from whvi_amd.layers import WHVILinear
    from whvi_amd.networks import WHVIRegression
    kinds = {"ReLU": nn.ReLU, "Sigmoid": nn.Sigmoid, "Tanh": nn.Tanh}
    for (na, a), (nb, b) in itertools.permutations(kinds.items(), 2):
        net = WHVIRegression([WHVILinear(3, 64), a(), WHVILinear(64, 64), b(), WHVILinear(64, 1)])
        reason = fused_mlp.match(net)
        assert isinstance(reason, str) and na in reason and nb in reason, (na, nb, reason)
    for (na, a), (nb, b) in itertools.permutations(kinds.items(), 2):          # two kinds side by side at one boundary
        reason = fused_mlp.match(WHVIRegression([WHVILinear(3, 64), a(), b(), WHVILinear(64, 64), WHVILinear(64, 1)]))
        assert isinstance(reason, str) and na in reason and nb in reason, (na, nb, reason)
    net = WHVIRegression([WHVILinear(1, 64), nn.Sigmoid(), WHVILinear(64, 64), nn.Sigmoid(), WHVILinear(64, 64), nn.Tanh(),
                          WHVILinear(64, 1)])
    assert "Tanh" in fused_mlp.match(net) and "Sigmoid" in fused_mlp.match(net)
    for cls in (nn.Sigmoid, nn.Tanh):
        assert "Cosine" in fused_mlp.match(WHVIRegression([WHVILinear(1, 64), cls(), WHVILinear(64, 64), Cosine(),
                                                            WHVILinear(64, 1)]))
        name = cls.__name__
        for mods in ([cls(), WHVILinear(3, 64), WHVILinear(64, 64), WHVILinear(64, 1)],
                     [WHVILinear(3, 64), WHVILinear(64, 64), WHVILinear(64, 1), cls()],
                     [WHVILinear(3, 64), cls(), cls(), WHVILinear(64, 64), WHVILinear(64, 1)]):
            reason = fused_mlp.match(WHVIRegression(mods))
            assert isinstance(reason, str) and name in reason and "between two WHVI layers" in reason, reason
    assert "Cosine" in fused_mlp.match(_net(3, 128, act=Cosine))


def test_training_plan_names_its_reasons_for_smooth_networks():
    from whvi_amd import _hip, fused_mlp
    net = _smooth_net(1, 128, 1, 3, nn.Sigmoid)
    assert "CUDA" in fused_mlp.plan(net, torch.randn(5, 1), 4, training=True)
    with torch.no_grad():
        assert "CUDA" in fused_mlp.plan(net, torch.randn(5, 1), 4)
    p = fused_mlp.match(_smooth_net(3, 2048, 1, 3, nn.Tanh))
    assert isinstance(p, fused_mlp.Plan) and not _hip.mlp_apply_bwd_supported(p.kind, len(p.mids), p.D)


# the dispatch of whvi_mlp_apply_act_f32 / _bwd_f32 (mlp_smooth_apply.hip, mlp_smooth_apply_bwd.hip), restated
def _forward_reached():
    from whvi_amd import _hip
    return {f"whvi::mlp_smooth_apply_kernel<float, {log2d}, {kin}, {act}>"
            for log2d in range(6, 12) for kin in (1, 4, 8) for act in (2, 3)
            if any(_hip.mlp_apply_supported(kin, n, 1 << log2d) for n in range(1, 5))}


def _backward_reached():
    from whvi_amd import _hip
    return {f"whvi::mlp_smooth_apply_bwd_kernel<float, {log2d}, {kin}, {n_mid}, {act}>"
            for log2d in range(6, 12) for kin in (1, 4, 8) for n_mid in (1, 2, 3, 4) for act in (2, 3)
            if _hip.mlp_apply_bwd_supported(kin, n_mid, 1 << log2d)}


def test_shipped_library_holds_the_smooth_kernels_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from shipped_isa import ShippedLibrary
    with ShippedLibrary() as lib:
        fwd = {n for n in lib.kernels if n.startswith("whvi::mlp_smooth_apply_kernel<")}
        bwd = {n for n in lib.kernels if n.startswith("whvi::mlp_smooth_apply_bwd_kernel<")}
        assert fwd == _forward_reached() and len(fwd) == 34
        assert bwd == _backward_reached() and len(bwd) == 60
        for name in fwd:
            k = lib.find(name)
            log2d = int(name.split(", ")[1])
            assert k["scratch"] == 0, name
            # the ReLU forward's budget: two waves per SIMD up to D = 1024, one at D = 2048
            assert k["vgprs"] + k["agprs"] <= (256 if log2d <= 10 else 512), (name, k["vgprs"], k["agprs"])
        for name in bwd:
            k = lib.find(name)
            log2d, kin, n_mid = (int(v) for v in name.split("<")[1].split(", ")[1:4])
            assert k["scratch"] == 0, name
            # the ReLU backward's budget (tests/test_mlp_train_host.py): two waves per SIMD except where its accumulators do
            # not allow it
            one_wave = (kin == 8 and n_mid == 2) or (log2d >= 9 and (kin == 8 or n_mid == 2))
            assert k["vgprs"] + k["agprs"] <= (512 if one_wave else 256), (name, k["vgprs"], k["agprs"])
        # the ReLU families are untouched (tests/test_mlp_apply_host.py, tests/test_mlp_train_host.py pin their counts)
        assert len([n for n in lib.kernels if n.startswith("whvi::mlp_apply_kernel<")]) == 17
        assert len([n for n in lib.kernels if n.startswith("whvi::mlp_apply_bwd_kernel<")]) == 30


def test_flags_change_nothing_on_host_tensors():
    for cls in (nn.Sigmoid, nn.Tanh):
        for n_in in (3, 1):
            torch.manual_seed(0)
            net = _smooth_net(n_in, 64, 1, 3, cls)
            net.eval_samples = 3
            net.train_samples = 2
            x, y = torch.randn(7, n_in), torch.randn(7, 1)
            net.eval()
            torch.manual_seed(1)
            want = net(x)
            net.set_fused_inference(True)
            torch.manual_seed(1)
            assert torch.equal(net(x), want)
            net.set_fused_inference(False)
            net.train()
            results = []
            for on in (False, True):
                net.set_fused_training(on)
                net.zero_grad(set_to_none=True)
                torch.manual_seed(2)
                loss = net.loss(x, y, n=7)
                loss.backward()
                results.append((loss.detach().clone(), [p.grad.clone() for p in net.parameters() if p.grad is not None]))
            (l0, g0), (l1, g1) = results
            assert torch.equal(l0, l1) and len(g0) == len(g1) > 0 and all(torch.equal(a, b) for a, b in zip(g0, g1))


def test_toy_sigmoid_reference_fixture_on_the_host(monkeypatch):
    """tests/golden/toy_sigmoid_golden.npz (the reference's own notebook model) through the host's batched route; the GPU file
    replays it through the fused passes."""
    from test_mlp_smooth_gpu import run_toy_sigmoid_fixture
    assert run_toy_sigmoid_fixture("cpu", monkeypatch, False) == []
