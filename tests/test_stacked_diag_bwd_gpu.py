"""whvi_diag_apply_stacked_bwd_f32 (whvi_amd/csrc/diag_apply_stacked_bwd.hpp) and the route built on it
(``WHVIStackedMatrix.diag_blocks_backward``, ``WHVINetwork.set_stacked_diagonal(backward=True)``): the backward of the stacked
diagonal launch in one call.

Checked over tools/stacked_diag_bwd_cases.py (a) ``grad_x`` bit for bit against the composition of existing launches
(``_hip.diag_apply_bwd`` per block, added in ascending j), with the buffers' guards untouched; (b) every element of ``out``
against float64 within gamma * 2^-24 * sum|terms|, gamma read off the launch's summation tree; (c) on the one launch large
enough to stream; (d) that the case list launches every shipped instantiation; (e) layer by layer and (f) network by network
against float64 autograd and the torch-op backward; (g) that the backward holds no temporary of activation size; (h) a
captured and replayed training step."""
import functools
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from whvi_amd import _hip, graphs
from whvi_amd.layers import WHVILinear
from whvi_amd.networks import WHVIRegression
from whvi_amd.weights import DiagApplyFunction, StackedDiagApplyFunction, WHVIStackedMatrix

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import stacked_diag_bwd_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRAD_TOL = 1e-5          # of max|ref| per tensor: the existing layer test's tolerance for these gradients
BWD = "whvi::stacked_diag_bwd_kernel<"


@functools.lru_cache(maxsize=None)
def _run(case):
    """One launch of a case into guarded buffers, and what it must equal: computed once, shared."""
    ops = bc.operands(case, DEV)
    gx, out, guarded, n_slabs = bc.launch(case, *ops)
    kernel = _hip.last_kernel()
    want_gx = bc.composed_grad_x(case, *ops) if case.need_gx else None
    ref, terms = bc.reference_out(case, *ops)
    torch.cuda.synchronize()
    return ops, gx, out, guarded, n_slabs, kernel, want_gx, ref, terms


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_grad_x_equals_the_composed_launches_bit_for_bit(case):
    (g, x, s1, s2, u, bias), gx, out, guarded, n_slabs, kernel, want, _, _ = _run(case)
    x3 = x if x.dim() == 3 else x.unsqueeze(0)
    assert (x3[:, 0, 0] == 0).all() and torch.signbit(x3[:, 0, 0]).all() and not torch.signbit(x3[:, 0, 1]).any()
    assert torch.isfinite(x).all() and (case.ld_out == case.n_cols or torch.isnan(g[..., case.n_cols:]).all())
    assert kernel == bc.kernel_symbol(case)
    assert bc.guards_untouched(guarded), "the launch wrote outside grad_x, out or part"
    if not case.need_gx:
        return
    assert gx.shape == want.shape == (case.S, case.B, case.D)
    assert torch.equal(gx, want), (kernel, int((gx != want).sum()))
    if case.n_cols < case.D:
        assert (gx[..., case.n_cols:] == 0).all() and not torch.signbit(gx[..., case.n_cols:]).any()      # +0 where no column reaches
    # (one row with relu_in: that row's x is the -0 / +0 pair, and its whole gradient is masked)
    assert torch.isfinite(gx).all() and ((gx != 0).any() or (case.B == 1 and case.relu_in))


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_out_against_float64_per_element(case):
    _, _, out, _, n_slabs, kernel, _, ref, terms = _run(case)
    m = 1 if case.mean_plus else 0
    got = out[:, :, m:].double()                 # (row 0 of a mean_plus out is the caller's)
    ref, terms = ref[:, :, m:], terms[:, :, m:]
    n = bc.gamma(case, n_slabs)
    gamma = n * 2.0 ** -24 / (1.0 - n * 2.0 ** -24)
    err, bound = (got - ref).abs(), gamma * terms
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{bc.case_id(case)}: {n_slabs} slabs, gamma = {n} u, max error / bound = {worst:.3f}")
    assert torch.isfinite(got).all() and (err <= bound).all(), (kernel, worst)
    # columns from n_cols on: zeros in all four slots
    flat = got.transpose(1, 2).reshape(4, got.shape[2], case.J * case.D)
    assert (flat[..., case.n_cols:] == 0).all()
    if case.B == 1:
        # one row: the bias slot is that row's masked g, and slots 0 - 2 are single products
        assert torch.equal(got[3], ref[3])


def test_unaligned_g_takes_the_dword_loads():
    case = bc.BwdCase(128, 2, 256, 256, 3, 37, False, True, True, True, True, 0, True)
    g, x, s1, s2, u, bias = bc.operands(case, DEV)
    shifted = torch.empty(g.numel() + 1, device=DEV)[1:].view_as(g).copy_(g)      # 4-byte aligned only
    assert shifted.data_ptr() % 16 == 4
    a = bc.launch(case, g, x, s1, s2, u, bias)
    b = bc.launch(case, shifted, x, s1, s2, u, bias)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][:, :, 1:], b[1][:, :, 1:]) and bc.guards_untouched(b[2])


def test_streaming_launch_takes_the_non_temporal_stores():
    case = bc.STREAM_CASE
    ops = bc.operands(case, DEV)
    gx, out, guarded, _ = bc.launch(case, *ops)
    assert _hip.last_kernel() == "whvi::stacked_diag_bwd_kernel<float, 1, true, true>"
    assert gx.numel() * 4 > 256 << 20 and bc.guards_untouched(guarded)
    want = bc.composed_grad_x(case, *ops)
    assert torch.equal(gx, want) and (gx[..., case.n_cols:] == 0).all()
    del gx, want, guarded
    small = case._replace(B=case.B - 100)
    bc.launch(small, *bc.operands(small, DEV))
    assert _hip.last_kernel() == "whvi::stacked_diag_bwd_kernel<float, 1, false, true>"


def test_case_list_launches_every_shipped_instantiation():
    from shipped_isa import ShippedLibrary
    seen = {_run(case)[5] for case in bc.CASES}
    with ShippedLibrary() as lib:
        shipped = {n for n in lib.kernels if n.startswith(BWD)}
    assert seen == shipped, (sorted(shipped - seen), sorted(seen - shipped))


def test_wrapper_takes_a_pitched_grad_out_and_matches_the_abi_call():
    case = bc.BwdCase(64, 3, 133, 140, 3, 37, True, True, True, True, True, 0, True)
    g, x, s1, s2, u, bias = bc.operands(case, DEV)
    gx, out, _, _ = bc.launch(case, g, x, s1, s2, u, bias)
    kw = dict(n_samples=case.S, n_cols=case.n_cols, mean_plus=True, bias=bias, relu_in=True, relu_out=True)
    gx2, out2 = _hip.diag_apply_stacked_bwd(g[..., :case.n_cols], x, s1, s2, u, **kw)          # a column slice: its own pitch
    assert torch.equal(gx, gx2) and torch.equal(out[:, :, 1:], out2[:, :, 1:])
    gx3, out3 = _hip.diag_apply_stacked_bwd(g[..., :case.n_cols].transpose(0, 1).contiguous().transpose(0, 1), x, s1, s2, u, **kw)
    assert torch.equal(gx, gx3) and torch.equal(out[:, :, 1:], out3[:, :, 1:])                 # no single pitch: made contiguous
    none, out4 = _hip.diag_apply_stacked_bwd(g[..., :case.n_cols], x, s1, s2, u, need_grad_x=False, **kw)
    assert none is None and torch.equal(out[:, :, 1:], out4[:, :, 1:])


# ---- the layer ---------------------------------------------------------------------------------------------------------
LAYERS = ((16, 128), (128, 2), (100, 100), (128, 512), (3, 64))


def _layer(n_in, n_out, backward, seed=7):
    torch.manual_seed(seed)
    layer = WHVIStackedMatrix(n_in, n_out, bias=True).to(DEV)
    with torch.no_grad():
        layer.bias.normal_()
        for m in layer.weight_matrices:
            m.s1.mul_(30.0)
            m.s2.mul_(30.0)
            m.g_mu.normal_()
    layer.diag_blocks, layer.diag_blocks_backward = True, backward
    return layer


def _layer_input(n_in, S, B, seed=9):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, B, n_in, generator=g) if n_in == 3 else torch.randn(B, n_in, generator=g)     # 3 -> 64: per-sample input
    x[..., 0, 0], x[..., 0, 1] = -0.0, 0.0
    return x.to(DEV)


def _stacked_params(layer):
    return [torch.stack([getattr(m, name) for m in layer.weight_matrices]) for name in ("s1", "s2", "g_mu", "g_rho")]


def _stacked_grads(layer):
    return [torch.stack([getattr(m, name).grad for m in layer.weight_matrices]) for name in ("s1", "s2", "g_mu", "g_rho")] + [layer.bias.grad]


def _stacked_ops(x, s1, s2, g_mu, g_rho, bias, eps, n_in, n_out, relu_in, relu_out):
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
def test_layer_forward_and_gradients(shape, relus, monkeypatch):
    S, B = 3, 37
    launches = []
    native = _hip.diag_apply_stacked_bwd
    monkeypatch.setattr(_hip, "diag_apply_stacked_bwd", lambda *a, **k: (launches.append(k["n_cols"]), native(*a, **k))[1])
    n_in, n_out = shape
    x0 = _layer_input(n_in, S, B)
    cot = torch.randn(S, B, n_out, generator=torch.Generator().manual_seed(4)).to(DEV)
    outs, grads = [], []
    for backward in (False, True):
        layer = _layer(*shape, backward)
        x = x0.clone().requires_grad_()
        torch.manual_seed(31)
        out = layer.forward_mc(x, S, relu_in=relus, relu_out=relus)
        (out * cot).sum().backward()
        assert launches == ([shape[1]] if backward else [])          # the one launch, or the torch ops
        outs.append(out.detach())
        grads.append([x.grad] + _stacked_grads(layer))
    assert torch.equal(outs[0], outs[1])
    layer = _layer(*shape, False)
    torch.manual_seed(31)
    eps = torch.randn(layer.stack, S, layer.D_in, device=DEV)
    ops = [t.detach().double().requires_grad_() for t in [x0] + _stacked_params(layer) + [layer.bias]]
    want = torch.autograd.grad((_stacked_ops(*ops, eps, n_in, n_out, relus, relus) * cot.double()).sum(), ops)
    for name, off, on, ref in zip(("x", "s1", "s2", "g_mu", "g_rho", "bias"), grads[0], grads[1], want):
        assert on.shape == off.shape
        _close(on, ref, f"{shape} {name} vs float64")
        _close(on, off, f"{shape} {name} vs the torch-op backward")


def test_layer_create_graph_with_the_flag_on_matches_the_flag_off_route():
    S, B, n_in, n_out = 3, 37, 100, 100
    cot = torch.randn(S, B, n_out, generator=torch.Generator().manual_seed(4)).to(DEV)
    res = []
    for backward in (False, True):
        layer = _layer(n_in, n_out, backward)
        x = _layer_input(n_in, S, B).requires_grad_()
        params = [p for n, p in layer.named_parameters() if n != "bias"]
        torch.manual_seed(33)
        out = layer.forward_mc(x, S, relu_in=True, relu_out=True)
        first = torch.autograd.grad((out * cot).sum(), [x] + params, create_graph=True)
        assert all(g.requires_grad for g in first)
        sum((g * g).sum() for g in first).backward()
        res.append([g.detach() for g in first] + [x.grad.clone()] + _stacked_grads(layer)[:4])
    for a, b in zip(*res):
        assert torch.equal(a, b)           # the same ops on the same mask (finite data)


# ---- networks ------------------------------------------------------------------------------------------------------------
def _net(n_in, backward, seed=5, S=8):
    torch.manual_seed(seed)
    net = WHVIRegression([WHVILinear(n_in, 128, bias=True), nn.ReLU(), WHVILinear(128, 128, bias=True), nn.ReLU(),
                          WHVILinear(128, 2, bias=True)], train_samples=S, eval_samples=S).to(DEV)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith((".s1", ".s2")):
                p.mul_(10.0)
            elif name.endswith(".g_mu") or name.endswith(".bias"):
                p.normal_()
    return net.set_stacked_diagonal(True, backward=backward)


def _net_ops(net, x, S, params, eps):
    first, last = net.sequential[0].weight_submodule, net.sequential[4].weight_submodule

    def stacked(prefix, layer, h, e, relu_in, relu_out):
        st = [torch.stack([params[f"{prefix}.weight_matrices.{j}.{n}"] for j in range(layer.stack)]) for n in ("s1", "s2", "g_mu", "g_rho")]
        return _stacked_ops(h, *st, params[f"{prefix}.bias"], e, layer.n_in, layer.n_out, relu_in, relu_out)

    h = stacked("sequential.0.weight_submodule", first, x, eps[0], False, True)
    p = "sequential.2.weight_submodule."
    u = torch.cat((params[p + "g_mu"].unsqueeze(0), F.softplus(params[p + "g_rho"]).unsqueeze(0) * eps[1][0].to(h.dtype)), dim=0)
    h = DiagApplyFunction._reference_ops(h, params[p + "s1"], params[p + "s2"], u, params[p + "bias"], True, False, True)
    return stacked("sequential.4.weight_submodule", last, h, eps[2], False, False).permute(1, 2, 0)


@pytest.mark.parametrize("n_in", (8, 16), ids=("energy", "naval"))
def test_network_loss_and_gradients(n_in):
    S, B = 8, 37
    g = torch.Generator().manual_seed(41)
    x, y = torch.randn(B, n_in, generator=g).to(DEV), torch.randn(B, 2, generator=g).to(DEV)
    cot = torch.randn(B, 2, S, generator=g).to(DEV)
    res = []
    for backward in (False, True):
        net = _net(n_in, backward).train()
        torch.manual_seed(43)
        loss = net.loss(x, y, n=1000)
        loss.backward()
        loss_grads = {n_: p.grad.clone() for n_, p in net.named_parameters()}
        net.zero_grad()
        torch.manual_seed(43)
        (net.forward_batched(x, S) * cot).sum().backward()
        res.append((loss.detach(), loss_grads, {n_: p.grad.clone() for n_, p in net.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0])                      # the forward is the same launch either way
    for name in res[0][1]:
        _close(res[1][1][name], res[0][1][name], f"loss gradient {name} vs the torch-op backward")
    net = _net(n_in, False)
    torch.manual_seed(43)
    layers = [net.sequential[i].weight_submodule for i in (0, 2, 4)]
    eps = [torch.randn(getattr(m, "stack", 1), S, getattr(m, "D_in", 128), device=DEV) for m in layers]
    params = {n_: p.detach().double().requires_grad_() for n_, p in net.named_parameters() if n_.startswith("sequential")}
    want = torch.autograd.grad((_net_ops(net, x.double(), S, params, eps) * cot.double()).sum(), list(params.values()))
    for (name, _), ref in zip(params.items(), want):
        _close(res[1][2][name], ref, f"gradient {name} vs float64")
        _close(res[1][2][name], res[0][2][name], f"gradient {name} vs the torch-op backward")


def test_output_layer_backward_holds_no_temporary_of_activation_size():
    S, B = 4, 512
    peaks = []
    for backward in (False, True):
        torch.manual_seed(47)
        layer = WHVILinear(1024, 2, bias=True).to(DEV)
        layer.weight_submodule.diag_blocks, layer.weight_submodule.diag_blocks_backward = True, backward
        h = torch.randn(S, B, 1024, device=DEV, requires_grad=True)
        out = layer.forward_mc(h, S, relu_in=True)
        loss = out.sum() + layer._mc_kl
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss.backward()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        assert _hip.last_kernel() != "" and h.grad is not None and h.grad.shape == h.shape
        del layer, h, out, loss
    act = S * B * 1024 * 4
    msg = (f"WHVILinear(1024, 2), {S} x {B} rows, backward(): peak above the graph's tensors {peaks[0] / 2 ** 20:.2f} MiB with the "
           f"torch ops, {peaks[1] / 2 ** 20:.2f} MiB with the launch; one activation is {act / 2 ** 20:.0f} MiB")
    print(msg)
    assert peaks[1] < peaks[0], msg
    assert peaks[1] < 2 * act, msg          # grad_x itself and nothing else of its size


def test_training_steps_captured_and_replayed():
    """The naval network at batch 64 with both flags on: three steps replayed from a captured graph end with the parameters of
    three eager steps of a twin on the same draws (compared the way test_fused_gpu.py compares a replay with an eager step)."""
    import copy
    B, steps = 64, 3
    g = torch.Generator().manual_seed(51)
    xs, ys = torch.randn(steps, B, 16, generator=g).to(DEV), torch.randn(steps, B, 2, generator=g).to(DEV)
    net = _net(16, True).train()
    twin = copy.deepcopy(net)
    assert all(m.diag_blocks and m.diag_blocks_backward for m in twin.modules() if isinstance(m, WHVIStackedMatrix))
    opt = torch.optim.Adam(net.parameters(), lr=1e-2, capturable=True)
    opt2 = torch.optim.Adam(twin.parameters(), lr=1e-2, capturable=True)
    before = [p.detach().clone() for p in net.parameters()]
    step = graphs.GraphedTrainStep(net, opt, xs[0], ys[0], n=1000)
    assert all(torch.equal(p.detach(), b) for p, b in zip(net.parameters(), before))
    dev = torch.device(DEV)
    rng = torch.cuda.get_rng_state(dev)
    losses = []
    for i in range(steps):
        torch.cuda.set_rng_state(rng, dev)
        loss_graph = float(step(xs[i], ys[i]))
        torch.cuda.set_rng_state(rng, dev)
        opt2.zero_grad(set_to_none=True)
        loss_eager = twin.loss(xs[i], ys[i], n=1000)
        loss_eager.backward()
        assert _hip.last_kernel() != ""
        opt2.step()
        losses.append((loss_graph, float(loss_eager.detach())))
        del loss_eager
    torch.cuda.synchronize()
    for a, b in losses:
        assert abs(a - b) <= 1e-6 * abs(b), losses
    moved = 0
    for (k, a), (_, b), c in zip(net.named_parameters(), twin.named_parameters(), before):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-7), k
        moved += int(not torch.equal(a.detach(), c))
    assert moved > 0
