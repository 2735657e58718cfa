"""The trainable one-launch pass of fastfood networks (WHVINetwork.set_fused_training: whvi_mlp_fastfood_apply_f32 forward,
whvi_mlp_fastfood_apply_bwd_f32 backward) on the GPU: the loss and the forward output bit for bit the batched route's, none of
the batched route's launches, every gradient tensor within 1e-5 of its largest float64 value on both routes for every shipped
instantiation, bit-equal gradients on every run, the batched route's non-finite pattern, the fallbacks, hipGraph training, and
not one byte written outside the outputs and the workspace.

Gradient yardstick: the network in float64 with torch autograd from the same float32 operands (dense H from
``whvi_amd.utils.build_H``), ReLU signs taken from the float32 forward of the batched route, one sample at a time; per gradient
tensor ``max|got - ref64| <= 1e-5 max|ref64|``.  The batched route is held to the same bound on the same cases."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

from whvi_amd import _hip, fastfood, fused_fastfood, weights
from whvi_amd.utils import build_H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mlp_apply_gpu import SENT, _placed  # noqa: E402
from test_mlp_fastfood_gpu import _net, _same  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
BWD = "whvi::mlp_fastfood_apply_bwd_kernel<"


class _BwdKernels:
    """The kernel each ``_hip.mlp_fastfood_apply_bwd`` call inside the block launched, read on the thread that made the call
    (autograd runs the backward on a thread of its own, and ``whvi_last_kernel`` is per thread)."""

    def __enter__(self):
        self.seen, self.inner = [], _hip.mlp_fastfood_apply_bwd

        def wrapped(*a, **k):
            out = self.inner(*a, **k)
            self.seen.append(_hip.last_kernel())
            return out
        _hip.mlp_fastfood_apply_bwd = wrapped
        return self.seen

    def __exit__(self, *exc):
        _hip.mlp_fastfood_apply_bwd = self.inner


def _loss_grads(net, x, y, S, fused, seed=1, x_grad=False):
    """One training pass (loss + backward) with the flag ``fused``: (loss, forward output, parameter gradients, grad_x)."""
    net.train()
    net.train_samples = S
    net.set_fused_training(fused)
    if any(getattr(m, "inkernel_rng", False) for m in net.modules()):
        net.set_inkernel_rng(True)              # a fresh generator, seeded from torch's below
    net.zero_grad(set_to_none=True)
    xx = x.detach().clone().requires_grad_(x_grad)
    torch.manual_seed(seed)
    out = net(xx)
    torch.manual_seed(seed)
    loss = net.loss(xx, y, n=x.shape[0])
    xx.grad = None
    with _BwdKernels() as seen:
        loss.backward()
    assert len(seen) == (1 if fused else 0) and all(k.startswith(BWD) for k in seen), seen
    grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    return loss.detach(), out.detach(), grads, (xx.grad.clone() if x_grad else None)


def _data(n_in, B, seed=2):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(B, n_in, device=DEV, generator=g), torch.randn(B, 1, device=DEV, generator=g)


def _close(a, b, what, rtol=1e-3):
    """Parameter gradients of the two routes: the same summands in a different summation order."""
    assert a.shape == b.shape, what
    scale = float(b.abs().max())
    assert float((a - b).abs().max()) <= rtol * scale + 1e-30, (what, float((a - b).abs().max()), scale)


NETS = {"toy": (1, 128, "sigmoid", 100, 1), "uci": (6, 128, "relu", 64, 1), "config4": (3, 1024, "relu", 256, 1),
        "config4_mc": (3, 1024, "relu", 2000, 16)}


# ---- routing: fails without the feature
@pytest.mark.parametrize("name", ["toy", "uci", "config4"])
def test_training_pass_takes_none_of_the_batched_launches(name, monkeypatch, hip_lib):
    n_in, D, act, B, S = NETS[name]

    def boom(*a, **k):
        raise AssertionError("the fused training pass took a batched launch")
    for cls in (fastfood.FastfoodFunction, weights.SmallKApplyFunction, weights.RowDotFunction):
        monkeypatch.setattr(cls, "apply", boom)
    monkeypatch.setattr(_hip, "fused_shs", boom)
    calls = []
    fwd = _hip.mlp_fastfood_apply
    monkeypatch.setattr(_hip, "mlp_fastfood_apply", lambda *a, **k: (calls.append("fwd"), fwd(*a, **k))[1])
    net = _net(n_in, D, act=act).train().set_fused_training(True)
    net.train_samples = 4
    x, y = _data(n_in, B)
    loss = net.loss(x, y, n=B)
    with _BwdKernels() as seen:
        loss.backward()
    kin = 1 if n_in == 1 else (4 if n_in <= 4 else 8)
    code = _hip.MLP_ACTS[act]
    # one forward launch; one backward call = the backward + its finishing launch
    assert calls == ["fwd"] and seen == [f"{BWD}float, {D.bit_length() - 1}, {kin}, 1, {code}>"], (calls, seen)
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    assert net._pass_kl is None


# ---- contract 1: forward and loss bit for bit
@pytest.mark.parametrize("name", sorted(NETS))
def test_loss_and_output_are_the_batched_routes(name, hip_lib):
    n_in, D, act, B, S = NETS[name]
    net = _net(n_in, D, act=act)
    x, y = _data(n_in, B)
    l0, o0, g0, x0 = _loss_grads(net, x, y, S, False, x_grad=True)
    l1, o1, g1, x1 = _loss_grads(net, x, y, S, True, x_grad=True)
    _same(o1, o0)
    _same(l1, l0)
    assert set(g0) == set(g1) and len(g0) == len(list(net.parameters()))
    for k in g0:
        _close(g1[k], g0[k], k)
    _close(x1, x0, "x")


@pytest.mark.parametrize("act", ["relu", "sigmoid", "tanh"])
@pytest.mark.parametrize("n_mid", [1, 2])
def test_every_bias_and_activation_pattern(n_mid, act, hip_lib):
    x, y = _data(3, 333)
    for bias_bits in range(1 << (n_mid + 2)):
        for act_bits in (range(1 << (n_mid + 1)) if bias_bits in (0, (1 << (n_mid + 2)) - 1) else (bias_bits % (1 << (n_mid + 1)),)):
            net = _net(3, 128, n_mid=n_mid, act=act, bias=[bool((bias_bits >> i) & 1) for i in range(n_mid + 2)],
                       acts=[bool((act_bits >> i) & 1) for i in range(n_mid + 1)])
            l0, o0, g0, _ = _loss_grads(net, x, y, 3, False)
            l1, o1, g1, _ = _loss_grads(net, x, y, 3, True)
            _same(o1, o0)
            _same(l1, l0)
            assert set(g0) == set(g1)             # (the gradients' yardstick is float64, at the operand level: below)


# ---- contract 2: gradients against float64
def _operands(kin, D, n_mid, S, B, biases, seed):
    """tests/test_mlp_train_gpu.py::_operands with every sample's g_k in place of u."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=g)  # noqa: E731
    ops = {"x": rnd(B, kin), "w_in": rnd(S, D) if kin == 1 else rnd(S, D, kin), "b_in": rnd(D) * 0.3 if biases[0] else None,
           "s1": rnd(n_mid, D), "s2": rnd(n_mid, D), "g": rnd(n_mid, S, D) * 0.3 / D,
           "b_mid": rnd(n_mid, D) * 0.3 if any(biases[1:-1]) else None, "w_out": rnd(S, D), "b_out": rnd(1) if biases[-1] else None}
    mid_bias = sum(1 << m for m in range(n_mid) if biases[1 + m])
    return ops, mid_bias, rnd(S, B)


def _leaves(ops, need_x):
    return {k: (None if v is None else v.detach().clone().requires_grad_(k != "x" or need_x)) for k, v in ops.items()}


_TORCH_ACT = {"relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}


def _batched_grads(ops, gy, mid_bias, bits, act, S, need_x):
    """The batched route's autograd Functions and torch ops, composed as forward_batched composes them for a fastfood
    network: the stacked first layer and the row dot fold their ReLU, every other activation is a torch op."""
    leaves = _leaves(ops, need_x)
    x, w_in, b_in = leaves["x"], leaves["w_in"], leaves["b_in"]
    n_mid, D = ops["s1"].shape
    B = x.shape[0]
    f = _TORCH_ACT[act]
    if w_in.dim() == 2:
        h = x * w_in.unsqueeze(1)
        if b_in is not None:
            h = h + b_in
        if bits & 1:
            h = f(h)
    else:
        h = weights.SmallKApplyFunction.apply(x, w_in, b_in, bool(bits & 1) and act == "relu")
        if bits & 1 and act != "relu":
            h = f(h)
    relu_in = False
    for m in range(n_mid):
        h = fastfood.FastfoodFunction.apply(h.reshape(S * B, D).contiguous(), leaves["s1"][m], leaves["g"][m], leaves["s2"][m],
                                            S, B).view(S, B, D)
        if (mid_bias >> m) & 1:
            h = h + leaves["b_mid"][m]
        if (bits >> (m + 1)) & 1:
            if act == "relu" and m == n_mid - 1:
                relu_in = True
            else:
                h = f(h)
    yv = weights.RowDotFunction.apply(h, leaves["w_out"], relu_in)
    if leaves["b_out"] is not None:
        yv = yv + leaves["b_out"]
    yv = yv.view(S, -1)
    yv.backward(gy)
    return yv.detach(), {k: (None if v is None else v.grad) for k, v in leaves.items()}


def _fused_grads(ops, gy, mid_bias, bits, act, need_x):
    leaves = _leaves(ops, need_x)
    yv = fused_fastfood.FastfoodMLPApplyFunction.apply(leaves["x"], leaves["w_in"], leaves["b_in"], leaves["s1"], leaves["s2"],
                                                       leaves["g"], leaves["b_mid"], leaves["w_out"], leaves["b_out"], mid_bias,
                                                       bits, act)
    with _BwdKernels() as seen:
        yv.backward(gy)
    n_mid, D = ops["s1"].shape
    kin = 1 if ops["w_in"].dim() == 2 else ops["w_in"].shape[2]
    assert seen == [f"{BWD}float, {D.bit_length() - 1}, {kin}, {n_mid}, {_hip.MLP_ACTS[act]}>"], seen
    return yv.detach(), {k: (None if v is None else v.grad) for k, v in leaves.items()}


def _ref64(ops, gy, mid_bias, bits, act, S):
    """float64 autograd of the network from the same float32 operands, one sample at a time (config 4's share is 3 GB per
    float32 activation); at a ReLU boundary both precisions differentiate the same piecewise-linear function: the sign
    pattern is the float32 forward's (the batched route's launches)."""
    n_mid, D = ops["s1"].shape
    x32 = ops["x"]
    B = x32.shape[0]
    H = build_H(D, DEV).double()
    lv = {k: (None if v is None else v.detach().double().requires_grad_(True)) for k, v in ops.items()}
    col = ops["w_in"].dim() == 2
    for s in range(S):
        masks = []
        with torch.no_grad():                                  # the float32 forward of the batched route: the ReLU signs
            if act == "relu":
                if col:
                    h = x32 * ops["w_in"][s]
                    h = h + ops["b_in"] if ops["b_in"] is not None else h
                else:
                    h = _hip.small_k_apply(x32, ops["w_in"][s:s + 1].contiguous(), ops["b_in"])[0]
                masks.append(h > 0)
                h = torch.relu(h) if bits & 1 else h
                for m in range(n_mid):
                    h = _hip.fused_shs(h.contiguous(), ops["s1"][m], ops["g"][m, s:s + 1].contiguous(), ops["s2"][m], axis="col",
                                       n_samples=1, sample_stride=B)
                    if (mid_bias >> m) & 1:
                        h = h + ops["b_mid"][m]
                    masks.append(h > 0)
                    h = torch.relu(h) if (bits >> (m + 1)) & 1 else h

        def activate(h, i):
            if not (bits >> i) & 1:
                return h
            return h * masks[i] if act == "relu" else _TORCH_ACT[act](h)
        x = lv["x"]
        h = x * lv["w_in"][s] if col else x @ lv["w_in"][s].t()
        if lv["b_in"] is not None:
            h = h + lv["b_in"]
        h = activate(h, 0)
        for m in range(n_mid):
            h = lv["s1"][m] * (((lv["g"][m, s] * ((lv["s2"][m] * h) @ H))) @ H)
            if (mid_bias >> m) & 1:
                h = h + lv["b_mid"][m]
            h = activate(h, m + 1)
        yv = h @ lv["w_out"][s]
        if lv["b_out"] is not None:
            yv = yv + lv["b_out"]
        yv.backward(gy[s].double())
    return {k: (None if v is None else v.grad) for k, v in lv.items()}


def _ratios(grads, ref, ops, mid_bias, need_x):
    """{tensor: max|got - ref64| / max|ref64|} over the gradient tensors of the pass."""
    n_mid = ops["s1"].shape[0]
    out = {}
    for k, v in ops.items():
        if v is None or (k == "x" and not need_x):
            continue
        got, want = grads[k], ref[k]
        if k == "b_mid":                        # layers without a bias: the fused pass sums their (unused) gradient too
            rows = [m for m in range(n_mid) if (mid_bias >> m) & 1]
            got = (got if got is not None else torch.zeros_like(v))[rows]
            want = want[rows]
        scale = float(want.abs().max())
        assert scale > 0, k
        out[k] = float((got.double().reshape(want.shape) - want).abs().max()) / scale
    return out


def _check_ratio(kin, D, n_mid, S, B, biases, bits, act, need_x, seed, batched=True):
    ops, mid_bias, gy = _operands(kin, D, n_mid, S, B, biases, seed)
    ref = _ref64(ops, gy, mid_bias, bits, act, S)
    yf, gf = _fused_grads(ops, gy, mid_bias, bits, act, need_x)
    worst = {"fused": _ratios(gf, ref, ops, mid_bias, need_x)}
    if batched:
        yb, gb = _batched_grads(ops, gy, mid_bias, bits, act, S, need_x)
        _same(yf, yb.contiguous())
        worst["batched"] = _ratios(gb, ref, ops, mid_bias, need_x)
        if not need_x:
            assert gf["x"] is None and gb["x"] is None
    for route, r in worst.items():
        print(f"ratio {route} K={kin} D={D} n_mid={n_mid} S={S} B={B} {act} bits={bits}: "
              + " ".join(f"{k}={v:.2e}" for k, v in r.items()))
    for route, r in worst.items():
        for k, v in r.items():
            assert v <= TOL, (route, k, v)
    return worst


def _ratio_cases():
    """Every shipped instantiation (K, D, n_mid, activation kind), with rotating row counts (not multiples of the slab or of
    the rows per iteration), sample counts 1 .. 7, bias and activation patterns, with and without grad_x."""
    rows = (1, 3, 257, 777, 1025)
    cases, i = [], 0
    for act in ("relu", "sigmoid", "tanh"):
        for log2d in range(6, 11):
            for kin in (1, 4, 8):
                for n_mid in (1, 2):
                    if not _hip.mlp_fastfood_apply_bwd_supported(kin, n_mid, 1 << log2d):
                        continue
                    full = (1 << (n_mid + 1)) - 1
                    bits = full if i % 3 else (i // 3) % (full + 1)
                    if act != "relu" and bits == 0:
                        bits = full                                # no activated boundary would launch the ReLU kernel
                    biases = tuple(bool((i >> j) & 1) or i % 4 == 0 for j in range(n_mid + 2))
                    cases.append((kin, log2d, n_mid, 1 + i % 7, rows[i % 5], biases, bits, act, i % 5 != 2))
                    i += 1
    return cases


@pytest.mark.parametrize("kin,log2d,n_mid,S,B,biases,bits,act,need_x", _ratio_cases())
def test_gradients_against_float64(kin, log2d, n_mid, S, B, biases, bits, act, need_x, hip_lib):
    _check_ratio(kin, 1 << log2d, n_mid, S, B, biases, bits, act, need_x, seed=7 + log2d * 13 + kin)


@pytest.mark.parametrize("kin,D,n_mid,S,B,act,bits", [
    (4, 1024, 1, 2, 4096, "relu", 3), (4, 1024, 2, 2, 2048, "relu", 7), (1, 128, 1, 1, 100, "sigmoid", 3),
    (8, 128, 2, 3, 1000, "relu", 7), (4, 1024, 1, 2, 4096, "relu", 0), (4, 512, 2, 2, 3000, "sigmoid", 7)])
def test_gradients_against_float64_named_shapes(kin, D, n_mid, S, B, act, bits, hip_lib):
    _check_ratio(kin, D, n_mid, S, B, (True,) * (n_mid + 2), bits, act, True, seed=3)


def test_config4_share_full_size(monkeypatch, hip_lib):
    """45 730 rows x 16 samples at D = 1024: the fused route inside the float64 bound (the batched route's ratios are printed,
    DESIGN 5.3g records them), the pass's peak memory above what is allocated before it under 256 MiB, and one forward and one
    backward call."""
    ops, mid_bias, gy = _operands(4, 1024, 1, 16, 45730, (True, True, True), 11)
    ref = _ref64(ops, gy, mid_bias, 3, "relu", 16)
    _, gf = _fused_grads(ops, gy, mid_bias, 3, "relu", True)
    fused = _ratios(gf, ref, ops, mid_bias, True)
    del gf
    _, gb = _batched_grads(ops, gy, mid_bias, 3, "relu", 16, True)
    batched = _ratios(gb, ref, ops, mid_bias, True)
    del gb, ref, ops, gy
    print("ratio fused config-4 share:", " ".join(f"{k}={v:.2e}" for k, v in fused.items()))
    print("ratio batched config-4 share:", " ".join(f"{k}={v:.2e}" for k, v in batched.items()))
    for k, v in fused.items():
        assert v <= TOL, (k, v)
    torch.cuda.empty_cache()
    net = _net(3, 1024)
    x, y = _data(3, 45730)
    net.train()
    net.train_samples = 16
    net.set_fused_training(True)
    calls = []
    fwd = _hip.mlp_fastfood_apply
    monkeypatch.setattr(_hip, "mlp_fastfood_apply", lambda *a, **k: (calls.append("fwd"), fwd(*a, **k))[1])

    def boom(*a, **k):
        raise AssertionError("a batched launch")
    for name in ("fused_shs", "small_k_apply", "row_dot"):
        monkeypatch.setattr(_hip, name, boom)
    for _ in range(2):                           # warm, then measure
        del calls[:]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss = net.loss(x, y, n=45730)
        with _BwdKernels() as seen:
            loss.backward()
        calls += ["bwd"] * len(seen)
        del loss
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    print("peak MiB", peak / 2 ** 20)
    assert peak < 256 << 20, peak / 2 ** 20
    assert calls == ["fwd", "bwd"]               # three launches: the forward, the backward and its finishing launch


# ---- contracts 3 and 4
def test_gradients_are_deterministic(hip_lib):
    net = _net(3, 1024)
    x, y = _data(3, 20000)
    runs = [_loss_grads(net, x, y, 8, True, x_grad=True) for _ in range(2)]
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    assert torch.equal(runs[0][3], runs[1][3])


@pytest.mark.parametrize("n_in,D,n_mid,act", [(3, 128, 1, "relu"), (1, 256, 2, "relu"), (6, 128, 2, "relu"), (1, 128, 1, "sigmoid"),
                                             (3, 1024, 1, "relu"), (3, 128, 2, "tanh")])
def test_non_finite_rows_give_the_batched_pattern(n_in, D, n_mid, act, hip_lib):
    net = _net(n_in, D, n_mid=n_mid, act=act)
    x, y = _data(n_in, 300)
    x[7, 0] = float("inf")
    x[13, 0] = float("-inf")
    x[100, n_in - 1] = float("nan")
    _, o0, g0, x0 = _loss_grads(net, x, y, 3, False, x_grad=True)
    _, o1, g1, x1 = _loss_grads(net, x, y, 3, True, x_grad=True)
    _same(o1, o0)
    for k in g0:
        assert torch.equal(torch.isfinite(g1[k]), torch.isfinite(g0[k])), k
    assert torch.equal(torch.isfinite(x1), torch.isfinite(x0))


# ---- packed parameters, in-kernel RNG
@pytest.mark.parametrize("packed,inkernel", [(True, False), (False, True), (True, True)])
def test_packed_parameters_and_inkernel_rng(packed, inkernel, hip_lib):
    net = _net(6, 256, n_mid=2)
    if packed:
        net.pack_parameters()
    if inkernel:
        net.set_inkernel_rng(True)
    x, y = _data(6, 300)
    l0, o0, g0, x0 = _loss_grads(net, x, y, 4, False, x_grad=True)
    l1, o1, g1, x1 = _loss_grads(net, x, y, 4, True, x_grad=True)
    _same(o1, o0)
    _same(l1, l0)
    assert set(g0) == set(g1)
    for k in g0:
        _close(g1[k], g0[k], k)
    _close(x1, x0, "x")


# ---- where the training pass does not apply
def test_double_backward_raises(hip_lib):
    net = _net(3, 128).train().set_fused_training(True)
    x, y = _data(3, 50)
    loss = net.loss(x, y, n=50)
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(loss, list(net.parameters()), create_graph=True)


@pytest.mark.parametrize("n_in,D,n_mid,modes,dtype", [(1, 2048, 1, None, None), (3, 128, 3, None, None), (6, 1024, 2, None, None),
                                                      (3, 128, 2, ["fastfood", "reference"], None), (1, 128, 1, None, torch.float64)])
def test_outside_the_range_takes_the_batched_route(n_in, D, n_mid, modes, dtype, monkeypatch, hip_lib):
    net = _net(n_in, D, n_mid=n_mid, modes=modes)
    x, y = _data(n_in, 64)
    if dtype is not None:
        net, x, y = net.to(dtype), x.to(dtype), y.to(dtype)
    l0, o0, g0, _ = _loss_grads(net, x, y, 2, False)

    def boom(*a, **k):
        raise AssertionError("the fused training pass ran outside its range")
    monkeypatch.setattr(_hip, "mlp_fastfood_apply_bwd", boom)
    monkeypatch.setattr(_hip, "mlp_fastfood_apply", boom)
    net.train()
    net.train_samples = 2
    net.set_fused_training(True)
    net.zero_grad(set_to_none=True)
    torch.manual_seed(1)
    o1 = net(x).detach()
    torch.manual_seed(1)
    l1 = net.loss(x, y, n=64)
    l1.backward()
    assert isinstance(fused_fastfood.plan(net, x, 2, training=True), str)
    assert torch.equal(o1, o0) and torch.equal(l1.detach(), l0)
    for k, p in net.named_parameters():
        assert torch.equal(p.grad, g0[k]), k


def test_inference_flag_alone_still_falls_back_when_a_graph_is_wanted(monkeypatch, hip_lib):
    net = _net(6, 128).set_fused_inference(True)

    def boom(*a, **k):
        raise AssertionError("a grad-wanting pass took a fused route without set_fused_training")
    monkeypatch.setattr(_hip, "mlp_fastfood_apply_bwd", boom)
    monkeypatch.setattr(_hip, "mlp_fastfood_apply", boom)
    x, y = _data(6, 50)
    net.train()
    loss = net.loss(x, y, n=50)
    loss.backward()
    assert torch.isfinite(loss)
    with torch.no_grad():
        assert "no autograd graph" in fused_fastfood.plan(net, x, 2, training=True)


# ---- hipGraph training
def _train(fused, seed=4):
    from whvi_amd.evaluation import make_optimizer
    from whvi_amd.layers import WHVILinear
    from whvi_amd.networks import WHVIRegression
    torch.manual_seed(seed)
    net = WHVIRegression([WHVILinear(3, 128, lambda_=3.0), nn.ReLU(), WHVILinear(128, 128, lambda_=3.0, mode="fastfood"), nn.ReLU(),
                          WHVILinear(128, 1, lambda_=3.0)]).to(DEV).train()
    net.train_samples = 2
    net.set_fused_training(fused)
    init = {k: v.clone() for k, v in net.state_dict().items()}
    X, Y = _data(3, 24, seed=5)
    loader = DataLoader(TensorDataset(X, Y), batch_size=8)
    optimizer, scheduler = make_optimizer(net, lambda0=0.05, capturable=True)
    losses = []

    seen = {"i": 0}

    def before_replay(step):
        if seen["i"] > 0:
            losses.append(step.static_loss.clone())
        seen["i"] += 1
    torch.manual_seed(seed + 100)
    step = net.train_model(loader, optimizer, scheduler, epochs1=2, epochs2=3, graphed=True,
                           graph_options={"before_replay": before_replay})
    losses.append(step.static_loss.clone())
    return init, torch.stack(losses), net.state_dict()


@pytest.mark.filterwarnings("error:The AccumulateGrad node's stream does not match:UserWarning")
def test_graphed_training_with_the_flag(hip_lib):
    init, loss_b, state_b = _train(False)
    _, loss_c, state_c = _train(False)
    # control: the seed pins the draws of a graphed run -- two flag-off runs reproduce each other bit for bit
    _same(loss_c, loss_b)
    for k in state_b:
        _same(state_c[k], state_b[k])
    _, loss_g, state_g = _train(True)
    steps = loss_g.shape[0]
    assert loss_g.shape == loss_b.shape and steps >= 14
    _same(loss_g[:1], loss_b[:1])                # the first replayed loss: the same draws, the same forward launch's values
    assert float((loss_g - loss_b).abs().max()) <= 1e-4 * float(loss_b.abs().max())
    lr_sum = sum(0.05 * 0.05 * (1 + 0.0005 * t) ** -0.3 for t in range(15))
    for k in state_g:
        ref, start, ours = state_b[k].double(), init[k].double(), state_g[k].double()
        moved = max(float((ref - start).abs().max()), lr_sum)
        assert float((ours - ref).abs().max()) <= 2e-2 * moved + 4e-7 * float(ref.abs().max()), k


# ---- buffers
def _cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        log2d, kin, n_mid = int(rng.integers(6, 11)), int(rng.choice([1, 4, 8])), int(rng.integers(1, 3))
        if _hip.mlp_fastfood_apply_bwd_supported(kin, n_mid, 1 << log2d):
            out.append((len(out), log2d, kin, n_mid, int(rng.integers(1, 6)), int(rng.integers(1, 1200))))
    return out


@pytest.mark.parametrize("case,log2d,kin,n_mid,S,B", _cases(12, 8))
def test_stays_inside_its_buffers(case, log2d, kin, n_mid, S, B, hip_lib):
    rng = np.random.default_rng(2000 + case)
    D = 1 << log2d
    ops, mid_bias, g = _operands(kin, D, n_mid, S, B, [bool(rng.integers(0, 2)) for _ in range(n_mid + 2)], seed=case)
    bits = int(rng.integers(0, 1 << (n_mid + 1)))
    act = ("relu", "sigmoid", "tanh")[case % 3]
    placed = {k: (None, None) if v is None else _placed(v, rng) for k, v in list(ops.items()) + [("gy", g)]}
    before = {k: b.clone() for k, (b, _) in placed.items() if b is not None}
    need = int(_hip.lib().whvi_mlp_fastfood_apply_bwd_workspace(S, B, kin, n_mid, log2d))
    outs = {"gwi": (S, D) if kin == 1 else (S, D, kin), "gs1": (n_mid, D), "gs2": (n_mid, D), "gg": (n_mid, S, D), "gwo": (S, D),
            "gb": ((1 + n_mid) * D + 1,), "gx": (S, B, kin), "work": (need,)}
    bufs = {k: _placed(torch.full(shape, SENT, device=DEV), rng) for k, shape in outs.items()}
    ptr = lambda k: None if placed[k][1] is None else placed[k][1].data_ptr()  # noqa: E731
    optr = lambda k: bufs[k][1].data_ptr()  # noqa: E731

    def call(work_floats):
        return _hip.lib().whvi_mlp_fastfood_apply_bwd_f32(
            optr("gwi"), optr("gs1"), optr("gs2"), optr("gg"), optr("gwo"), optr("gb"), optr("gx"), optr("work"), work_floats,
            ptr("gy"), ptr("x"), kin, ptr("w_in"), ptr("b_in"), n_mid, ptr("s1"), ptr("s2"), ptr("g"), ptr("b_mid"), mid_bias,
            ptr("w_out"), S, B, log2d, _hip.MLP_ACTS[act], bits, None)
    assert call(need - 1) == -1 and "workspace" in _hip.last_error()       # one float too small: WHVI_ERR_ARG, no launch
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert bool((buf == SENT).all()), k
    rc = call(need)
    torch.cuda.synchronize()
    assert rc == 0, _hip.last_error()
    for k, (buf, view) in bufs.items():
        off = (view.data_ptr() - buf.data_ptr()) // 4
        assert bool((buf[:off] == SENT).all()) and bool((buf[off + view.numel():] == SENT).all()), k
        if k != "work":
            assert bool((view != SENT).all()), k
    for k, b in before.items():
        assert torch.equal(placed[k][0], b), k
    want = _hip.mlp_fastfood_apply_bwd(g, ops["x"], ops["w_in"], ops["b_in"], ops["s1"], ops["s2"], ops["g"], ops["b_mid"],
                                       ops["w_out"], mid_bias=mid_bias, act_bits=bits, need_grad_x=True, act=act)
    for k, w in zip(("gwi", "gs1", "gs2", "gg", "gwo", "gb", "gx"), want):
        _same(bufs[k][1], w)
