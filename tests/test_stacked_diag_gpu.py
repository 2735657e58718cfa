"""whvi_diag_apply_stacked_f32 (whvi_amd/csrc/diag_apply_stacked.hpp) and the route built on it
(``WHVIStackedMatrix.diag_blocks``, ``WHVINetwork.set_stacked_diagonal``): all diagonal blocks of a reference-mode stacked layer
written by one launch, bias, both ReLUs and the narrowing to ``n_out`` included.

Checked (a) bit for bit -- whole output, pad columns included -- against the composition of existing launches (``_hip.diag_apply``
per block, ``cat``, narrowing) over tools/stacked_diag_cases.py, with zeros of both signs, poisoned rows and non-finite
parameters in the operands; (b) per element against float64 on finite operands; (c) on the one launch large enough to stream;
(d) that the case list launches every shipped instantiation; (e) layer by layer and (f) network by network against today's
``WBarFunction`` + ``matmul`` route under one seed, values and gradients."""
import functools
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from whvi_amd import _hip
from whvi_amd.layers import WHVILinear
from whvi_amd.networks import WHVIRegression
from whvi_amd.weights import DiagApplyFunction, StackedDiagApplyFunction, WBarFunction, WHVIStackedMatrix

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import stacked_diag_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 12345.5
GRAD_TOL = 1e-5          # of max|ref| per tensor: the project's standing tolerance for these gradients


def _same_bits(a, b):
    """Every element bit-equal, or NaN in both."""
    return bool(((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)) | (a.isnan() & b.isnan())).all())


@functools.lru_cache(maxsize=None)
def _run(case):
    """One launch of a case into a sentinel-filled pitched buffer, and the composed launches: computed once, shared."""
    ops = sc.operands(case, DEV)
    buf = torch.full((case.S, case.B, case.ld_out), SENTINEL, device=DEV)
    sc.launch(case, *ops, out=buf[..., :case.n_cols])
    kernel = _hip.last_kernel()
    want = sc.composed(case, *ops)
    torch.cuda.synchronize()
    return ops, buf, want, kernel


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_launch_equals_the_composed_launches_bit_for_bit(case):
    (x, s1, s2, u, bias), buf, want, kernel = _run(case)
    # the operands hold what the check is about
    x3 = x if x.dim() == 3 else x.unsqueeze(0)
    assert (x3[:, 0, 0] == 0).all() and torch.signbit(x3[:, 0, 0]).all() and not torch.signbit(x3[:, 0, 1]).any()
    assert (s1 * s2 < 0).any() and torch.isinf(s1).sum() == 1 and float(u.abs().max()) > 1e38
    if case.B >= 4:
        bad = (~torch.isfinite(x3)).sum(dim=2)
        assert (bad[:, 1] == 1).all() and (bad[:, 2] == 1).all() and (bad[:, 3] == 2).all() and torch.isnan(x3[:, 2]).any()
    got = buf[..., :case.n_cols]
    assert got.shape == want.shape
    assert _same_bits(got, want), (kernel, int((got != want).sum()))
    assert (buf[..., case.n_cols:] == SENTINEL).all(), "columns n_cols .. ld_out - 1 were touched"
    if case.B >= 4:
        # the poison reached every block: rows 1 and 2 are NaN except at their one non-finite column (per block), row 3 everywhere
        nan = torch.isnan(got)
        assert nan[:, 3].all()
        keep = torch.arange(case.n_cols, device=DEV) % case.D
        assert nan[:, 1][:, keep != 2 % case.D].all() and nan[:, 2][:, keep != 1].all()


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_launch_against_float64_on_finite_operands(case):
    x, s1, s2, u, bias = sc.operands(case, DEV, special=False, seed=1)
    got = sc.launch(case, x, s1, s2, u, bias).cpu().double()
    x, s1, s2, u = (t.cpu().double() for t in (x, s1, s2, u))
    D = float(case.D)
    wd = s1.unsqueeze(1) * D * u * s2.unsqueeze(1)                        # (J, U, D)
    if case.mean_plus:
        w_mean, w_k = wd[:, :1].expand(-1, case.S, -1), wd[:, 1:]
    else:
        w_mean, w_k = torch.zeros_like(wd), wd
    xa = torch.relu(x) if case.relu_in else x
    x3 = (xa if xa.dim() == 3 else xa.unsqueeze(0)).unsqueeze(2)          # (S or 1, B, 1, D)
    flat = lambda t: t.reshape(t.shape[0], t.shape[1], case.J * case.D)[..., :case.n_cols]      # noqa: E731
    ref = flat(x3 * (w_mean + w_k).transpose(0, 1).unsqueeze(1))
    bound = 5.0 * flat(x3.abs() * (w_mean.abs() + w_k.abs()).transpose(0, 1).unsqueeze(1))
    if bias is not None:
        b = bias.cpu().double()[:case.n_cols]
        ref, bound = ref + b, bound + 2.0 * b.abs()
    if case.relu_out:
        ref = torch.relu(ref)
    err, bound = (got - ref).abs(), 2.0 ** -24 * bound
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{sc.case_id(case)}: max error / bound = {worst:.3f}")
    assert torch.isfinite(got).all() and (err <= bound).all(), worst


def test_streaming_launch_takes_the_non_temporal_stores():
    case = sc.STREAM_CASE
    ops = sc.operands(case, DEV)
    got = sc.launch(case, *ops)
    assert _hip.last_kernel() == "whvi::diag_apply_stacked_kernel<float, 4, true>"
    assert got.numel() * 4 > 256 << 20
    want = sc.composed(case, *ops)
    assert _same_bits(got, want)
    del got, want
    # one batch row less per slab of 100: below the threshold the cached stores are taken
    small = case._replace(B=case.B - 100)
    sc.launch(small, *sc.operands(small, DEV))
    assert _hip.last_kernel() == "whvi::diag_apply_stacked_kernel<float, 4, false>"


def test_case_list_launches_every_shipped_instantiation():
    from shipped_isa import ShippedLibrary
    seen = {_run(case)[3] for case in sc.CASES}
    with ShippedLibrary() as lib:
        shipped = {n for n in lib.kernels if n.startswith("whvi::diag_apply_stacked_kernel<")}
    assert seen == shipped, (sorted(shipped - seen), sorted(seen - shipped))


# ---- the layer ---------------------------------------------------------------------------------------------------------
LAYERS = ((16, 128), (128, 2), (100, 100), (128, 512), (3, 64))


def _layer(n_in, n_out, flag, seed=7):
    torch.manual_seed(seed)
    layer = WHVIStackedMatrix(n_in, n_out, bias=True).to(DEV)
    with torch.no_grad():
        layer.bias.normal_()
        for m in layer.weight_matrices:
            m.s1.mul_(30.0)
            m.s2.mul_(30.0)
            m.g_mu.normal_()
    layer.diag_blocks = flag
    return layer


def _layer_input(n_in, S, B, poisoned, seed=9):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, B, n_in, generator=g) if n_in == 3 else torch.randn(B, n_in, generator=g)     # 3 -> 64: per-sample input
    x[..., 0, 0], x[..., 0, 1] = -0.0, 0.0
    if poisoned:
        x[..., 1, 1] = float("inf")
        x[..., 2, 0] = float("nan")
        x[..., 3, 0], x[..., 3, n_in - 1] = float("inf"), float("-inf")
    return x.to(DEV)


def _same_values(a, b):
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


@pytest.mark.parametrize("relus", (False, True), ids=("plain", "relus"))
@pytest.mark.parametrize("poisoned", (False, True), ids=("finite", "poisoned"))
@pytest.mark.parametrize("shape", LAYERS, ids=lambda s: f"{s[0]}to{s[1]}")
def test_layer_forward_mc_equals_the_matrix_route(shape, poisoned, relus):
    S, B = 3, 37
    x = _layer_input(shape[0], S, B, poisoned)
    outs = []
    for flag in (False, True):
        layer = _layer(*shape, flag)
        assert layer._diag_blocks_route(x) is flag and layer.fuses_relu(x) is flag
        torch.manual_seed(21)
        with torch.no_grad():
            out = layer.forward_mc(x, S, relu_in=relus, relu_out=relus)
        assert _hip.last_kernel().startswith("whvi::diag_apply_stacked_kernel<") is flag
        torch.manual_seed(21)
        out_g = layer.forward_mc(x, S, relu_in=relus, relu_out=relus)          # the pass that wants a graph: same values, its KL
        assert _same_values(out, out_g.detach())
        outs.append((out, layer._mc_kl.detach()))
    assert outs[0][0].shape == (S, B, shape[1])
    assert _same_values(outs[0][0], outs[1][0]), int((outs[0][0] != outs[1][0]).sum())
    assert torch.isnan(outs[1][0]).any() == poisoned
    assert torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("shape", ((16, 128), (128, 2), (3, 64)), ids=lambda s: f"{s[0]}to{s[1]}")
def test_layer_forward_one_sample(shape):
    x = _layer_input(shape[0], 1, 37, False)
    x = x[0] if x.dim() == 3 else x
    outs = []
    for flag in (False, True):
        layer = _layer(*shape, flag)
        torch.manual_seed(23)
        with torch.no_grad():
            out = layer(x)
            assert _hip.last_kernel().startswith("whvi::diag_apply_stacked_kernel<") is flag
            outs.append((out, layer.kl))
    a, b = outs[0][0], outs[1][0]
    assert a.shape == b.shape == (37, shape[1])
    if shape[0] == 3:
        # K = 4: the GEMM's fused multiply-adds do not add the accumulator's + 0 the way the diagonal launch does
        ulp = torch.maximum(a.abs(), b.abs()) * 2.0 ** -23 + 1e-45
        assert ((a - b).abs() <= ulp).all()
    else:
        assert _same_values(a, b)
    assert torch.equal(outs[0][1], outs[1][1])


def _stacked_params(layer):
    return [torch.stack([getattr(m, name) for m in layer.weight_matrices]) for name in ("s1", "s2", "g_mu", "g_rho")]


def _stacked_grads(layer):
    return [torch.stack([getattr(m, name).grad for m in layer.weight_matrices]) for name in ("s1", "s2", "g_mu", "g_rho")] + [layer.bias.grad]


def _stacked_ops(x, s1, s2, g_mu, g_rho, bias, eps, n_in, n_out, relu_in, relu_out):
    """The layer's batched pass as differentiable torch ops, in the dtype of its arguments."""
    u = torch.cat((g_mu.unsqueeze(1), F.softplus(g_rho).unsqueeze(1) * eps.to(g_mu.dtype)), dim=1)
    xp = F.pad(x, (0, s1.shape[1] - n_in))
    return StackedDiagApplyFunction._reference_ops(xp, s1, s2, u, bias, n_out, True, relu_in, relu_out)


def _close(got, want, what):
    scale = float(want.abs().max())
    err = float((got.double() - want.double()).abs().max())
    print(f"{what}: max error {err:.3e}, max|ref| {scale:.3e}, ratio {err / max(scale, 1e-300):.2e}")
    assert err <= GRAD_TOL * scale, (what, err, scale)


@pytest.mark.parametrize("relus", (False, True), ids=("plain", "relus"))
@pytest.mark.parametrize("shape", LAYERS, ids=lambda s: f"{s[0]}to{s[1]}")
def test_layer_gradients(shape, relus):
    S, B = 3, 37
    n_in, n_out = shape
    x0 = _layer_input(n_in, S, B, False)
    cot = torch.randn(S, B, n_out, generator=torch.Generator().manual_seed(4)).to(DEV)
    grads = []
    for flag in (False, True):
        layer = _layer(*shape, flag)
        x = x0.clone().requires_grad_()
        torch.manual_seed(31)
        out = layer.forward_mc(x, S, relu_in=relus, relu_out=relus)
        (out * cot).sum().backward()
        grads.append([x.grad] + _stacked_grads(layer))
    # float64 autograd of the torch-ops expression, on the same draw
    layer = _layer(*shape, False)
    torch.manual_seed(31)
    eps = torch.randn(layer.stack, S, layer.D_in, device=DEV)
    ops = [t.detach().double().requires_grad_() for t in [x0] + _stacked_params(layer) + [layer.bias]]
    out = _stacked_ops(*ops, eps, n_in, n_out, relus, relus)
    want = torch.autograd.grad((out * cot.double()).sum(), ops)
    names = ("x", "s1", "s2", "g_mu", "g_rho", "bias")
    for name, off, on, ref in zip(names, grads[0], grads[1], want):
        _close(on, ref, f"{shape} {name} vs float64")
        _close(on, off, f"{shape} {name} vs the matrix route")


def test_layer_create_graph_runs_and_matches_the_ops():
    S, B, n_in, n_out = 3, 37, 100, 100
    layer = _layer(n_in, n_out, True)
    x = _layer_input(n_in, S, B, False).requires_grad_()
    cot = torch.randn(S, B, n_out, generator=torch.Generator().manual_seed(4)).to(DEV)
    params = [p for n, p in layer.named_parameters() if n != "bias"]
    torch.manual_seed(33)
    out = layer.forward_mc(x, S, relu_in=True, relu_out=True)
    first = torch.autograd.grad((out * cot).sum(), [x] + params, create_graph=True)
    assert all(g.requires_grad for g in first)
    sum((g * g).sum() for g in first).backward()              # the graph of the backward runs
    second_on = [x.grad.clone()] + _stacked_grads(layer)[:4]
    # the same two derivatives through the ops expression (the bias has no second derivative: its gradient is a sum of masks)
    layer2 = _layer(n_in, n_out, False)
    torch.manual_seed(33)
    eps = torch.randn(layer2.stack, S, layer2.D_in, device=DEV)
    ops = [t.detach().clone().requires_grad_() for t in [x] + _stacked_params(layer2)]
    out2 = _stacked_ops(*ops, layer2.bias.detach(), eps, n_in, n_out, True, True)
    _close(out.detach(), out2.detach(), "create_graph: forward")
    first2 = torch.autograd.grad((out2 * cot).sum(), ops, create_graph=True)
    second = torch.autograd.grad(sum((g * g).sum() for g in first2), ops)
    _close(first[0].detach(), first2[0].detach(), "create_graph: first-order grad_x")
    for name, got, ref in zip(("x", "s1", "s2", "g_mu", "g_rho"), second_on, second):
        _close(got, ref, f"create_graph: second-order {name}")


# ---- networks ------------------------------------------------------------------------------------------------------------
def _net(n_in, flag, seed=5):
    torch.manual_seed(seed)
    net = WHVIRegression([WHVILinear(n_in, 128, bias=True), nn.ReLU(), WHVILinear(128, 128, bias=True), nn.ReLU(),
                          WHVILinear(128, 2, bias=True)], train_samples=8, eval_samples=8).to(DEV)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith((".s1", ".s2")):
                p.mul_(10.0)
            elif name.endswith(".g_mu") or name.endswith(".bias"):
                p.normal_()
    return net.set_stacked_diagonal(flag)


def _net_ops(net, x, S, params, eps):
    """forward_batched of the 3-layer network as torch ops in the dtype of ``params`` (a dict name -> tensor)."""
    first, mid, last = net.sequential[0].weight_submodule, net.sequential[2].weight_submodule, net.sequential[4].weight_submodule

    def stacked(prefix, layer, h, e, relu_in, relu_out):
        st = [torch.stack([params[f"{prefix}.weight_matrices.{j}.{n}"] for j in range(layer.stack)]) for n in ("s1", "s2", "g_mu", "g_rho")]
        return _stacked_ops(h, *st, params[f"{prefix}.bias"], e, layer.n_in, layer.n_out, relu_in, relu_out)

    h = stacked("sequential.0.weight_submodule", first, x, eps[0], False, True)
    p = "sequential.2.weight_submodule."
    u = torch.cat((params[p + "g_mu"].unsqueeze(0), F.softplus(params[p + "g_rho"]).unsqueeze(0) * eps[1][0].to(h.dtype)), dim=0)
    h = DiagApplyFunction._reference_ops(h, params[p + "s1"], params[p + "s2"], u, params[p + "bias"], True, False, True)
    return stacked("sequential.4.weight_submodule", last, h, eps[2], False, False).permute(1, 2, 0)


@pytest.mark.parametrize("n_in", (8, 16), ids=("energy", "naval"))
def test_network_values_loss_and_gradients(n_in):
    S, B = 8, 37
    g = torch.Generator().manual_seed(41)
    x, y = torch.randn(B, n_in, generator=g).to(DEV), torch.randn(B, 2, generator=g).to(DEV)
    cot = torch.randn(B, 2, S, generator=g).to(DEV)
    res = []
    for flag in (False, True):
        net = _net(n_in, flag).train()
        torch.manual_seed(43)
        with torch.no_grad():
            out = net.forward_batched(x, S)
        torch.manual_seed(43)
        loss = net.loss(x, y, n=1000)
        loss.backward()
        loss_grads = {n_: p.grad.clone() for n_, p in net.named_parameters()}
        net.zero_grad()
        torch.manual_seed(43)
        (net.forward_batched(x, S) * cot).sum().backward()
        res.append((out, loss.detach(), loss_grads, {n_: p.grad.clone() for n_, p in net.named_parameters() if p.grad is not None}))
    assert res[0][0].shape == (B, 2, S) and _same_values(res[0][0], res[1][0])
    rel = abs(float(res[0][1]) - float(res[1][1])) / abs(float(res[0][1]))
    print(f"loss: flag off {float(res[0][1]):.6f}, on {float(res[1][1]):.6f}, relative difference {rel:.2e}")
    assert rel <= 1e-6
    for name in res[0][2]:
        _close(res[1][2][name], res[0][2][name], f"loss gradient {name} vs the matrix route")
    # float64 autograd of the torch-ops expression of the same pass, on the same draws (layer by layer, in order)
    net = _net(n_in, False)
    torch.manual_seed(43)
    layers = [net.sequential[i].weight_submodule for i in (0, 2, 4)]
    eps = [torch.randn(getattr(m, "stack", 1), S, getattr(m, "D_in", 128), device=DEV) for m in layers]
    params = {n_: p.detach().double().requires_grad_() for n_, p in net.named_parameters() if n_.startswith("sequential")}
    out = _net_ops(net, x.double(), S, params, eps)
    want = torch.autograd.grad((out * cot.double()).sum(), list(params.values()))
    for (name, _), ref in zip(params.items(), want):
        _close(res[1][3][name], ref, f"gradient {name} vs float64")
        _close(res[1][3][name], res[0][3][name], f"gradient {name} vs the matrix route")


def test_network_builds_no_matrix_with_the_flag_on(monkeypatch):
    S, B = 8, 37
    g = torch.Generator().manual_seed(45)
    x, y = torch.randn(B, 16, generator=g).to(DEV), torch.randn(B, 2, generator=g).to(DEV)
    net = _net(16, True).train()          # naval: the 16-feature first layer and the 2-target output layer are both stacked
    calls = []

    def refuse(*args):
        calls.append(args[1].shape)
        raise AssertionError("WBarFunction.apply: a weight matrix was built")

    monkeypatch.setattr(WBarFunction, "apply", refuse)
    net.loss(x, y, n=1000).backward()
    with torch.no_grad():
        net.forward_batched(x, S)
        net.eval()
        net(x)
    assert calls == [] and all(p.grad is not None for p in net.parameters())
    net.set_faithful_dataflow(True)
    with pytest.raises(AssertionError, match="a weight matrix was built"):
        net.forward_batched(x, S)
    assert len(calls) == 1


def test_output_layer_peak_memory_stays_below_one_weight_stack():
    S, B = 4, 512
    torch.manual_seed(47)
    layer = WHVILinear(1024, 2, bias=True).to(DEV)
    layer.weight_submodule.diag_blocks = True
    h = torch.randn(S, B, 1024, device=DEV, requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = layer.forward_mc(h, S, relu_in=True)
    (out.sum() + layer._mc_kl).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    stack = S * 1024 * 1024 * 4
    print(f"WHVILinear(1024, 2), {S} x {B} rows, forward + backward: peak {peak / 2 ** 20:.2f} MiB above the operands; "
          f"one (S, 1024, 1024) weight stack is {stack / 2 ** 20:.0f} MiB")
    assert _hip.last_kernel() != "" and out.shape == (S, B, 2) and h.grad is not None
    assert peak < stack
