"""One-launch passes of a WHVI regression network of the canonical shape: the predictive pass (opt-in:
``WHVINetwork.set_fused_inference()``) and the training pass, forward + backward (opt-in: ``WHVINetwork.set_fused_training()``).

The reference's networks -- ``[WHVILinear(n_in, D), act, WHVILinear(D, D), act, WHVILinear(D, 1)]``: the UCI networks with
``act = nn.ReLU`` (src/evaluation.py:79-85), the toy notebook's WHVI models 1 -> 128 -> 128 -> 1 with ``act = nn.Sigmoid``
(experiments/Toy example.ipynb), BASELINE config 4's 3 -> 1024 -> 1024 -> 1 with ReLU -- run on the batched GPU route as three
launches that write and re-read two ``(S, B, D)`` activations (plus one torch pass per sigmoid).  ``whvi_mlp_apply_f32``
(whvi_amd/csrc/mlp_apply.hpp) keeps each row's hidden vector on chip instead: it reads ``x`` and writes ``y``.  Each boundary
carries ``nn.ReLU``, ``nn.Sigmoid``, ``nn.Tanh`` or nothing, one activation kind per network (sigmoid and tanh through
``whvi_mlp_apply_act_f32``, ATen's float formulas).  Every layer's operands come from the same ``_mc_operands`` the batched
route's ``forward_mc`` calls, in the same order, so the draws are the same; the kernel repeats the arithmetic of the launches
it replaces, so the result is bit-identical to ``forward_batched`` without the flag.

Training: ``MLPApplyFunction`` wraps the same launch in an autograd Function that saves only its inputs.  Its backward is
one call of ``whvi_mlp_apply_bwd_f32`` (whvi_amd/csrc/mlp_apply_bwd.hpp), which recomputes every row's hidden vectors with the
forward's arithmetic -- hence the batched route's ReLU masks, or the sigmoid / tanh outputs torch's backward formulas read --
and applies that route's backward formulas; the batch sums run
in a fixed order (bit-identical gradients on every run).  They differ from the batched route's gradients only by summation
order; the loss is bit-identical.  The gradient w.r.t. each square layer's diagonal is chained to ``u``, ``s1`` and ``s2`` by
small torch ops, and autograd continues through ``_mc_operands`` to the parameters.  There is no double backward.

``match(net)`` is the structural check (no device needed), ``plan(net, x, n_samples[, training])`` adds the checks of one call,
``run`` makes the pass.  Both return a human-readable reason instead of a plan when the network or the call is not covered; the
caller then takes the batched route.  The predictive plan (``training=False``) refuses a call that wants an autograd graph;
the training plan (``training=True``) takes exactly those, within ``whvi_mlp_apply_bwd_f32``'s narrower range."""
from typing import List, NamedTuple, Optional, Union

import torch
import torch.nn as nn

from whvi_amd import _hip
from whvi_amd.layers import WHVILinear
from whvi_amd.weights import WHVIColumnMatrix, WHVISquarePow2Matrix, WHVIStackedMatrix

__all__ = ["Plan", "MLPApplyFunction", "match", "plan", "run"]


class Plan(NamedTuple):
    first: nn.Module                 # WHVIStackedMatrix (K = D_in = 4 / 8) or WHVIColumnMatrix (n_in = 1)
    kind: int                        # _hip.MLP_FIRST_K4 / _K8 / _COLUMN
    n_in: int
    mids: List[nn.Module]            # WHVISquarePow2Matrix, 1 .. 4 of them
    last: nn.Module                  # transposed WHVIColumnMatrix (D -> 1)
    layers: List[nn.Module]          # the WHVILinear modules in order (their _mc_kl is cleared like forward_batched does)
    D: int
    relu: int                        # ReLU networks: act_bits; sigmoid / tanh networks: 0
    act: str = "relu"                # the activation kind at every activated boundary: "relu", "sigmoid" or "tanh"
    act_bits: int = 0                # bit 0: the activation behind the first layer, bit 1 + m: behind square layer m


_ACTS = {nn.ReLU: "relu", nn.Sigmoid: "sigmoid", nn.Tanh: "tanh"}      # the activations the passes fuse


def _scan(net):
    """``(layers, act_after, act, act_mod)`` of ``net``'s module list -- its WHVILinear modules, whether an activation follows
    each, the one activation kind (or None) and its module name -- or why the fused passes cannot take that list."""
    mods = list(net.sequential)
    layers, relu_after = [], []
    act, act_mod = None, None
    for i, m in enumerate(mods):
        kind = _ACTS.get(type(m))
        if kind is not None:
            name = type(m).__name__
            if act is not None and kind != act:
                return f"module {i}: nn.{name} after nn.{act_mod}: the fused passes take one activation kind per network"
            if not layers or relu_after[-1] or i == len(mods) - 1:
                return f"module {i}: an nn.{name} is only fused between two WHVI layers (one per boundary)"
            act, act_mod = kind, name
            relu_after[-1] = True
        elif isinstance(m, WHVILinear):
            layers.append(m)
            relu_after.append(False)
        else:
            return f"module {i}: {type(m).__name__} is neither WHVILinear nor nn.ReLU / nn.Sigmoid / nn.Tanh"
    if len(layers) < 3:
        return f"{len(layers)} WHVI layers: the fused pass needs a first layer, 1 .. 4 square layers and an output layer"
    if len(layers) - 2 > 4:
        return f"{len(layers) - 2} square layers: at most 4"
    return layers, relu_after, act, act_mod


def _first_layer(first):
    """``(D, kind, n_in)`` of a first layer the fused passes take, or why not."""
    if isinstance(first, WHVIStackedMatrix):
        if first.D_in not in (4, 8):
            return f"first layer: {first.n_in} inputs pad to K = {first.D_in} (4 or 8 only)"
        D, kind, n_in = first.n_out, first.D_in, first.n_in
        if first.D_out != D:
            return f"first layer: {D} outputs are not a whole number of {first.D_in}-row blocks"
    elif isinstance(first, WHVIColumnMatrix) and not first.transposed:
        D, kind, n_in = first.D, _hip.MLP_FIRST_COLUMN, 1
        if first.D_adjusted != D:
            return f"first layer: hidden width {D} is not a power of two"
    else:
        return f"first layer: {type(first).__name__} is neither a stacked (K = 4 / 8) nor a column (n_in = 1) WHVI matrix"
    return D, kind, n_in


def _output_layer(last, D):
    """Why ``last`` is not the output layer the fused passes take (None when it is)."""
    if not (isinstance(last, WHVIColumnMatrix) and last.transposed):
        return f"output layer: {type(last).__name__} is not WHVILinear(D, 1) (one output only)"
    if last.D != D or last.weight_submodule.D != D:
        return f"output layer: width {last.D} differs from the hidden width {D}"
    return None


def _act_bits(relu_after) -> int:
    bits = 0
    for i, r in enumerate(relu_after[:-1]):
        bits |= (1 << i) if r else 0
    return bits


def match(net) -> Union[Plan, str]:
    """The plan of the one-launch pass for ``net``'s module list, or why it has none."""
    scan = _scan(net)
    if isinstance(scan, str):
        return scan
    layers, relu_after, act, _ = scan
    subs = [m.weight_submodule for m in layers]
    for i, w in enumerate(subs):
        if not isinstance(w, (WHVIStackedMatrix, WHVIColumnMatrix, WHVISquarePow2Matrix)):
            return f"layer {i}: {type(w).__name__} (mode='fastfood'?) is not a reference-mode WHVI matrix"
        if getattr(w, "hip_apply", True) is False:
            return f"layer {i}: faithful dataflow is on (hip_apply = False)"
    first, mids, last = subs[0], subs[1:-1], subs[-1]
    head = _first_layer(first)
    if isinstance(head, str):
        return head
    D, kind, n_in = head
    for j, w in enumerate(mids):
        if not isinstance(w, WHVISquarePow2Matrix):
            return f"layer {1 + j}: {type(w).__name__} is not a square power-of-two WHVI matrix (hidden width {D}?)"
        if w.D != D:
            return f"layer {1 + j}: width {w.D} differs from the first layer's {D}"
        if w._diag_mode() is False:
            return f"layer {1 + j}: faithful dataflow is on (the diagonal route is switched off)"
    reason = _output_layer(last, D)
    if reason is not None:
        return reason
    if not _hip.mlp_apply_supported(kind, len(mids), D):
        return f"hidden width {D} with {len(mids)} square layers is outside whvi_mlp_apply's range"
    bits = _act_bits(relu_after)
    act = act or "relu"
    return Plan(first, kind, n_in, mids, last, layers, D, bits if act == "relu" else 0, act, bits)


def _params(p: Plan):
    return [t for m in p.layers for t in m.parameters()]


def plan(net, x: torch.Tensor, n_samples: int, training: bool = False) -> Union[Plan, str]:
    """``match(net)`` plus the checks of this call: float32 CUDA input and parameters on x's device, sizes, and no autograd
    graph wanted (grad mode off, or neither x nor any parameter of the pass requires grad).  ``training=True``: the plan of the
    trainable pass instead -- the same checks, but a graph must be wanted and the network must lie in the backward's range
    (``_hip.mlp_apply_bwd_supported``)."""
    p = match(net)
    if isinstance(p, str):
        return p
    if x.device.type != "cuda" or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != p.n_in:
        return f"input: needs a float32 CUDA (batch, {p.n_in}) tensor"
    params = _params(p)
    if any(t.device != x.device or t.dtype != torch.float32 for t in params):
        return "parameters: float32 on the input's device only"
    S, B = int(n_samples), x.shape[0]
    if S < 1 or S * B >= 2 ** 32:
        return f"{S} samples x {B} rows: outside 1 .. 2^32 - 1 rows"
    wanted = torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in params))
    if not training:
        return "an autograd graph is wanted (the fused pass has no backward)" if wanted else p
    if not wanted:
        return "no autograd graph is wanted (the training pass is for passes that need one)"
    if not _hip.mlp_apply_bwd_supported(p.kind, len(p.mids), p.D):
        return f"hidden width {p.D} with {len(p.mids)} square layers is outside whvi_mlp_apply_bwd's range"
    return p


class MLPApplyFunction(torch.autograd.Function):
    """``y (S, B) = mlp_apply(x, w_in, b_in, s1, s2, u, b_mid, w_out, b_out)`` (whvi_mlp_apply_f32) with a backward: one call of
    ``whvi_mlp_apply_bwd_f32`` that recomputes the hidden vectors instead of reading saved ones (only the inputs are saved).
    ``s1, s2`` (n_mid, D), ``u`` (n_mid, 1 + S, D) as ``whvi_diag_apply``'s mean-plus layout; the gradient w.r.t. each sample's
    diagonal goes to ``u``, ``s1`` and ``s2`` with the formulas of ``whvi_diag_apply_bwd``'s finishing launch, row 0 of ``u``
    (the mean) taking the sum over the samples, as ``DiagApplyFunction.backward`` does.  First order only."""

    @staticmethod
    def forward(ctx, x, w_in, b_in, s1, s2, u, b_mid, w_out, b_out, mid_bias, relu, act="relu"):
        ctx.mid_bias, ctx.relu, ctx.act = int(mid_bias), int(relu), act
        ctx.save_for_backward(x, w_in, b_in, s1, s2, u, b_mid, w_out, b_out)
        return _hip.mlp_apply(x, w_in, b_in, s1, s2, u, b_mid, w_out, b_out, mid_bias=mid_bias, relu=relu, act=act)

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            raise RuntimeError("MLPApplyFunction: the fused training pass has no double backward -- call backward() without "
                               "create_graph=True, or turn WHVINetwork.set_fused_training off for this pass")
        x, w_in, b_in, s1, s2, u, b_mid, w_out, b_out = ctx.saved_tensors
        need = ctx.needs_input_grad
        gw_in, gw_mid, gw_out, gb, gx = _hip.mlp_apply_bwd(g, x, w_in, b_in, s1, s2, u, b_mid, w_out, mid_bias=ctx.mid_bias,
                                                          relu=ctx.relu, need_grad_x=need[0], act=ctx.act)
        n_mid, S, D = gw_mid.shape
        grad_x = gx.sum(dim=0) if gx is not None else None
        grad_b_in = gb[:D].view(b_in.shape) if b_in is not None else None
        grad_b_mid = gb[D:(1 + n_mid) * D].view(b_mid.shape) if b_mid is not None else None
        grad_b_out = gb[(1 + n_mid) * D:].view(b_out.shape) if b_out is not None else None
        grad_s1 = grad_s2 = grad_u = None
        if need[3] or need[4] or need[5]:
            # d w_k / d (s1, s2, u) of w_k = wbar(u_0) + wbar(u_1+k) = s1 * D * (u_0 * s2) + s1 * D * (u_1+k * s2), per sample k
            Dd = float(D)
            a, c = s1.unsqueeze(1), s2.unsqueeze(1)
            u0, uk = u[:, :1], u[:, 1:]
            k_u = gw_mid * (a * Dd * c)                                           # (n_mid, S, D): dL/du_1+k
            grad_u = torch.cat((k_u.sum(dim=1, keepdim=True), k_u), dim=1)        # row 0 (the mean) takes the sum
            grad_s1 = (gw_mid * (Dd * (u0 * c) + Dd * (uk * c))).sum(dim=1)
            grad_s2 = (gw_mid * (a * Dd * (u0 + uk))).sum(dim=1)
        return grad_x, gw_in, grad_b_in, grad_s1, grad_s2, grad_u, grad_b_mid, gw_out, grad_b_out, None, None, None


def _bias(w) -> Optional[torch.Tensor]:
    return None if w.bias is None else w.bias.reshape(-1)


def run(net, p: Plan, x: torch.Tensor, n_samples: int, training: bool = False) -> torch.Tensor:
    """The pass: each layer's draws in module order (``_mc_operands``, as ``forward_mc`` makes them), then ONE launch
    (``training``: through ``MLPApplyFunction``, for a plan of ``plan(..., training=True)``).  Returns ``(batch, 1, S)`` in
    forward_batched's layout; sets ``net._pass_kl`` like the batched route does."""
    S = int(n_samples)
    first = p.first
    w_in, kl = first._mc_operands(S)                                # (S, D, K) or (S, D)
    kls = [kl]
    if p.kind == _hip.MLP_FIRST_COLUMN:
        xin = x
    else:
        xin = torch.zeros((x.shape[0], first.D_in), device=x.device)   # forward_mc's x_padded
        xin[:, :first.n_in] = x
    us = []
    for w in p.mids:
        u, kl = w._mc_operands(S)                                   # (1 + S, D)
        us.append(u)
        kls.append(kl)
    w_out, kl = p.last._mc_operands(S)                              # (S, D)
    kls.append(kl)
    for m in p.layers:
        m._mc_kl = None
        m.weight_submodule._mc_kl = None
    if len(p.mids) == 1:
        m0 = p.mids[0]
        s1, s2, u = m0.s1.unsqueeze(0), m0.s2.unsqueeze(0), us[0].unsqueeze(0)
    else:
        s1 = torch.stack([m.s1 for m in p.mids])
        s2 = torch.stack([m.s2 for m in p.mids])
        u = torch.stack(us)
    mid_bias = sum(1 << j for j, m in enumerate(p.mids) if m.bias is not None)
    b_mid = None
    if mid_bias:
        b_mid = torch.stack([m.bias.reshape(-1) if m.bias is not None else torch.zeros_like(m.s1) for m in p.mids])
    if training:
        y = MLPApplyFunction.apply(xin, w_in, _bias(first), s1, s2, u, b_mid, w_out, _bias(p.last), mid_bias, p.act_bits, p.act)
    else:
        y = _hip.mlp_apply(xin, w_in, _bias(first), s1, s2, u, b_mid, w_out, _bias(p.last), mid_bias=mid_bias, relu=p.act_bits,
                           act=p.act)
    total = None
    if all(torch.is_tensor(k) for k in kls):
        for k in kls:
            total = k if total is None else total + k
    net._pass_kl = total
    return y.unsqueeze(-1).permute(1, 2, 0)
