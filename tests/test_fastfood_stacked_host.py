"""The rectangular fastfood layer (whvi_fused_shs_stacked_f32, whvi_amd.fastfood.WHVIFastfoodStackedMatrix,
``WHVILinear(..., mode="fastfood_stacked")``) as far as it can be checked without a GPU: the ABI declares and exports the two
symbols, the support rule and its Python mirror, every refusal (ctypes with fake aligned pointers: the checks happen before
any device call), what the shipped library contains -- a fused_shs_stacked_kernel<float, L, ...> for every L in 6 .. 11, none
with scratch, and the unchanged sets of fused_shs_kernel / fused_shs_bwd_kernel symbols -- and, on host tensors, the Module
against the dense float64 product built with ``build_H``: pad, one diag(s1_j) H diag(g_{j,k}) H diag(s2_j) per block,
concatenate, narrow, add the bias."""
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from whvi_amd.layers import WHVILinear
from whvi_amd.networks import WHVIRegression
from whvi_amd.utils import build_H

from test_host import ReplayRandn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("whvi_fused_shs_stacked_supported", "whvi_fused_shs_stacked_f32")
SRC_SHARED = 4
MODE = "fastfood_stacked"


# ---- the dense float64 reference, shared with tests/test_fastfood_stacked_gpu.py ---------------------------------------------
def make_layer(n_in, n_out, bias=True, seed=0):
    """A layer in the new mode with parameters of order one (the initialisation's are 0.01 and 0)."""
    torch.manual_seed(seed)
    layer = WHVILinear(n_in, n_out, lambda_=0.7, bias=bias, mode=MODE)
    sub = layer.weight_submodule
    with torch.no_grad():
        for m in sub.weight_matrices:
            m.g_mu.copy_(torch.randn(sub.D_in) * 0.3)
            m.s1.mul_(10.0)
            m.s2.mul_(10.0)
        if bias:
            sub.bias.copy_(torch.randn(1, sub.D_out) * 0.1)
    return layer


def dense_reference(sub, x, eps):
    """``(y (S, B, n_out), leaves)`` in float64 with an autograd graph: ``x`` (B, n_in) or (S, B, n_in), ``eps`` (J, S, D_in);
    ``leaves`` = [x, then the parameters in ``sub.parameters()`` order] as float64 leaves on ``x``'s device."""
    J, D, S = sub.stack, sub.D_in, eps.size(1)
    xd = x.detach().double().requires_grad_()
    params = [p.detach().double().requires_grad_() for p in sub.parameters()]
    named = dict(zip((n for n, _ in sub.named_parameters()), params))
    H = build_H(D, x.device).double()
    xp = F.pad(xd, (0, D - sub.n_in))
    if xp.dim() == 2:
        xp = xp.unsqueeze(0).expand(S, -1, -1)
    outs = []
    for j in range(J):
        s1, s2 = named[f"weight_matrices.{j}.s1"], named[f"weight_matrices.{j}.s2"]
        g = named[f"weight_matrices.{j}.g_mu"] + F.softplus(named[f"weight_matrices.{j}.g_rho"]) * eps[j].double()    # (S, D)
        W = s1[None, :, None] * (H @ (g[:, :, None] * (H * s2[None, :])))                                               # (S, D, D)
        outs.append(torch.einsum("sbd,snd->sbn", xp, W))
    y = torch.cat(outs, dim=-1)
    if sub.bias is not None:
        y = y + named["bias"]
    return y[..., :sub.n_out], [xd] + params


def check_layer_against_dense(layer, x, S, monkeypatch, grad_tol=None, seed=5):
    """Forward and every gradient of ``layer.forward_mc(x, S)`` against the dense float64 product.  Forward bound: the one
    tests/test_fastfood.py uses, 2e-5 * max(1, D / 32) * max|want|; gradients: ``grad_tol`` (default: that file's, the same
    figure) times max|want| per tensor."""
    sub = layer.weight_submodule
    D = sub.D_in
    eps = torch.randn(sub.stack, S, D, generator=torch.Generator().manual_seed(seed))
    x = x.detach().requires_grad_()
    monkeypatch.setattr(torch, "randn", ReplayRandn([eps.numpy()]))
    y = layer.forward_mc(x, S)
    monkeypatch.undo()
    want, leaves = dense_reference(sub, x, eps.to(x.device))
    assert y.shape == want.shape == (S, x.size(-2), sub.n_out)
    w = torch.randn(want.shape, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64).to(x.device)
    tol = 2e-5 * max(1.0, D / 32)
    assert float((y.detach().double() - want.detach()).abs().max()) <= tol * float(want.detach().abs().max())
    got = torch.autograd.grad((y.double() * w).sum(), [x] + list(sub.parameters()))
    ref = torch.autograd.grad((want * w).sum(), leaves)
    names = ["x"] + [n for n, _ in sub.named_parameters()]
    gtol = tol if grad_tol is None else grad_tol
    for name, p, q in zip(names, got, ref):
        assert p.shape == q.shape, name
        assert float((p.double() - q).abs().max()) <= gtol * float(q.abs().max()), name
    return y.detach()


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_both_symbols():
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
    for log2d, J, want in ((5, 1, 0), (6, 1, 1), (11, 1, 1), (12, 1, 0), (6, 0, 0), (9, -1, 0),
                           (6, 85, 1), (6, 86, 0),            # 12 * 64 * 85 = 65280, * 86 = 66048
                           (10, 5, 1), (10, 6, 0),            # 12 * 1024 * 5 = 61440, * 6 = 73728
                           (11, 2, 1), (11, 3, 0)):           # 12 * 2048 * 2 = 49152, * 3 = 73728
        assert L.whvi_fused_shs_stacked_supported(log2d, J) == want, (log2d, J)
        assert _hip.fused_shs_stacked_supported(torch.float32, 1 << log2d, J) == bool(want), (log2d, J)
    for log2d in range(0, 16):
        for J in (1, 2, 3, 5, 6, 21, 22, 42, 43, 85, 86, 1 << 40):
            rule = 6 <= log2d <= 11 and 12 * (1 << log2d) * J <= 65536
            assert L.whvi_fused_shs_stacked_supported(log2d, J) == int(rule), (log2d, J)
            assert _hip.fused_shs_stacked_supported(torch.float32, 1 << log2d, J) == rule, (log2d, J)
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        assert not _hip.fused_shs_stacked_supported(dtype, 256, 2)
    assert not _hip.fused_shs_stacked_supported(torch.float32, 100, 2)


def test_refusals_before_any_device_call():
    from whvi_amd import _hip
    fn = _hip.lib().whvi_fused_shs_stacked_f32
    buf = (ctypes.c_char * (1 << 20))()
    p = (ctypes.addressof(buf) + 15) & ~15
    K = 65536                     # J = 2, S = 2, stride = 2, D = 512: dst 16 KiB, src 8 KiB (4 shared), a / c 4 KiB, b 8 KiB
    dst, src, a, b, c = (p + i * K for i in range(5))

    def call(dst=dst, src=src, a=a, b=b, c=c, J=2, S=2, stride=2, log2d=9, flags=0):
        return fn(dst, src, a, b, c, J, S, stride, log2d, flags, None)

    err = _hip.last_error
    assert call(flags=1) == -1 and "unknown fused flags" in err()
    assert call(flags=8) == -1 and "unknown fused flags" in err()
    assert call(flags=SRC_SHARED | 16) == -1 and "unknown fused flags" in err()
    for name in ("dst", "src", "a", "b", "c"):
        assert call(**{name: None}) == -1 and "null" in err(), name
    assert call(J=-1) == -1 and call(S=-1) == -1 and call(stride=-1) == -1
    for log2d in (-1, 0, 5, 12, 13):
        assert call(log2d=log2d) == -2 and "supported range" in err(), log2d
    assert call(J=0) == -2
    assert call(J=11) == -2 and "LDS" in err()                          # 12 * 512 * 11 > 65536
    assert call(J=10, S=0) == 0
    assert call(log2d=11, J=3) == -2 and call(log2d=6, J=86) == -2
    assert call(S=1 << 20, stride=1 << 12) == -2 and "32 bits" in err()
    for name, ptr in (("dst", dst), ("src", src), ("a", a), ("b", b), ("c", c)):
        assert call(**{name: ptr + 4}) == -3 and "aligned" in err(), name
    # dst (16 KiB) over each input
    assert call(dst=src) == -5 and "overlap" in err()
    assert call(dst=src + 8192 - 16) == -5 and call(dst=src - 16384 + 16) == -5
    assert call(dst=a + 4080) == -5 and call(dst=b + 8176) == -5 and call(dst=c - 16) == -5
    assert call(dst=src + 4096 - 16, flags=SRC_SHARED) == -5            # (a shared source is sample_stride rows: 4 KiB)
    # nothing to do: accepted without touching a pointer or a device
    assert call(S=0) == 0 and err() == ""
    assert call(stride=0) == 0 and err() == ""
    assert fn(None, None, None, None, None, 2, 0, 7, 9, 0, None) == 0
    assert fn(None, None, None, None, None, 1, 3, 0, 11, SRC_SHARED, None) == 0


def _shipped():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    return shipped_isa.ShippedLibrary()


def test_shipped_library_has_every_instantiation_and_keeps_the_pinned_symbol_sets():
    with _shipped() as lib:
        kernels = lib.kernels
    mine = {n: k for n, k in kernels.items() if n.startswith("whvi::fused_shs_stacked_kernel<")}
    want = {f"whvi::fused_shs_stacked_kernel<float, {L}, {8 if L == 11 else 4}, {nt}>" for L in range(6, 12) for nt in ("true", "false")}
    assert set(mine) == want
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgprs"] + k["agprs"] <= 256, (name, k)
    golden = [g for g in open(os.path.join(ROOT, "tests", "golden", "fused_shs_kernel_symbols_f32_f64.txt")).read().split("\n")
              if g.strip()]
    assert sorted(n for n in kernels if re.match(r"whvi::fused_shs_kernel<(float|double), ", n)) == sorted(golden)
    # the one-launch backward: float32 and the two 16-bit storage types, D = 64 .. 4096, cached and streaming
    k_of = {"float": (4, 4, 4, 4, 4, 8, 16), "__half": (2, 2, 2, 2, 2, 4, 8), "__hip_bfloat16": (2, 2, 2, 2, 2, 4, 8)}
    bwd = {f"whvi::fused_shs_bwd_kernel<{t}, {L}, {ks[L - 6]}, {nt}>" for t, ks in k_of.items() for L in range(6, 13)
           for nt in ("true", "false")}
    assert {n for n in kernels if n.startswith("whvi::fused_shs_bwd_kernel<")} == bwd


# ---- the Module on host tensors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(6, 16), (16, 40), (10, 16), (16, 3), (16, 16)])
def test_layer_against_the_dense_float64_product_cpu(n_in, n_out, monkeypatch):
    S, B = 3, 5
    layer = make_layer(n_in, n_out)
    sub = layer.weight_submodule
    assert type(sub).__name__ == "WHVIFastfoodStackedMatrix"
    D = 1 << (n_in - 1).bit_length()
    assert (sub.D_in, sub.stack, sub.padding, sub.D_out) == (D, -(-n_out // D), D - n_in, D * -(-n_out // D))
    gen = torch.Generator().manual_seed(3)
    y2 = check_layer_against_dense(layer, torch.randn(B, n_in, generator=gen), S, monkeypatch)
    check_layer_against_dense(layer, torch.randn(S, B, n_in, generator=gen), S, monkeypatch)
    assert y2.shape == (S, B, n_out)
    # one stochastic pass == sample 0 of the batched pass with the same draw
    x = torch.randn(B, n_in, generator=gen)
    eps = torch.randn(sub.stack, 1, D, generator=gen).numpy()
    with torch.no_grad():
        monkeypatch.setattr(torch, "randn", ReplayRandn([eps]))
        y1 = layer(x)
        monkeypatch.setattr(torch, "randn", ReplayRandn([eps]))
        y_mc = layer.forward_mc(x, 1)
        monkeypatch.undo()
    assert y1.shape == (B, n_out) and torch.equal(y1, y_mc[0])
    assert torch.equal(layer.kl, sum(m.kl for m in sub.weight_matrices))


def test_stacked_state_dict_loads_and_the_same_seed_gives_the_same_parameters():
    for n_in, n_out, bias in ((6, 16, True), (16, 40, False), (128, 512, True)):
        torch.manual_seed(11)
        ref = WHVILinear(n_in, n_out, lambda_=0.3, bias=bias)
        torch.manual_seed(11)
        new = WHVILinear(n_in, n_out, lambda_=0.3, bias=bias, mode=MODE)
        assert type(ref.weight_submodule).__name__ == "WHVIStackedMatrix"
        a, b = ref.state_dict(), new.state_dict()
        assert list(a) == list(b)
        for key in a:
            assert torch.equal(a[key], b[key]), key
        torch.manual_seed(12)
        other = WHVILinear(n_in, n_out, lambda_=0.3, bias=bias)
        new.load_state_dict(other.state_dict())
        for key, value in other.state_dict().items():
            assert torch.equal(new.state_dict()[key], value), key
        assert torch.allclose(new.kl, other.kl)


def test_the_other_modes_are_unchanged():
    with pytest.raises(ValueError):
        WHVILinear(3, 16, mode="fastfood")
    with pytest.raises(ValueError):
        WHVILinear(8, 8, mode="stacked")
    assert type(WHVILinear(8, 8).weight_submodule).__name__ == "WHVISquarePow2Matrix"
    assert type(WHVILinear(8, 8, mode="fastfood").weight_submodule).__name__ == "WHVIFastfoodMatrix"
    assert type(WHVILinear(3, 16).weight_submodule).__name__ == "WHVIStackedMatrix"
    assert type(WHVILinear(8, 8, mode=MODE).weight_submodule).__name__ == "WHVIFastfoodStackedMatrix"
    assert type(WHVILinear(1, 8, mode=MODE).weight_submodule).__name__ == "WHVIFastfoodStackedMatrix"


def test_network_in_the_new_mode():
    from whvi_amd import fused_fastfood, fused_mlp
    torch.manual_seed(0)
    S, B = 5, 12
    net = WHVIRegression([WHVILinear(6, 16, lambda_=1.0, mode=MODE), nn.ReLU(), WHVILinear(16, 32, lambda_=1.0, mode=MODE), nn.ReLU(),
                          WHVILinear(32, 2, lambda_=1.0, mode=MODE)], train_samples=3, eval_samples=S)
    x, y = torch.randn(B, 6), torch.randn(B, 2)
    for mode in ("loop", "batched"):
        net.mc_mode = mode
        net.train()
        net.zero_grad()
        loss = net.loss(x, y, n=100)
        loss.backward()
        assert torch.isfinite(loss)
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
        net.eval()
        assert net(x).shape == (B, 2, S)
    for match in (fused_mlp.match, fused_fastfood.match):
        reason = match(net)
        assert isinstance(reason, str) and "WHVIFastfoodStackedMatrix" in reason, reason
