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
the training plan (``training=True``) takes exactly those, within ``whvi_mlp_apply_bwd_f32``'s narrower range.  Everything that
does not depend on the kind of square layer -- the scan of the module list, the checks of a call, the draws and the launch --
is ``whvi_amd._fused_net``'s, shared with ``whvi_amd.fused_fastfood``; here are the diagonal layers' checks, their operands'
layout, the chain rule to ``u``, ``s1``, ``s2`` and the KL sum."""
from typing import List, NamedTuple, Union

import torch
import torch.nn as nn

from whvi_amd import _fused_net, _hip
from whvi_amd._fused_net import _act_bits, _first_layer, _output_layer, _scan
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


_KIND = _fused_net.Kind("fused pass", "square layers is outside whvi_mlp_apply_bwd's range", _hip.mlp_apply_bwd_supported)


def plan(net, x: torch.Tensor, n_samples: int, training: bool = False) -> Union[Plan, str]:
    """``match(net)`` plus the checks of this call (``_fused_net.check_call``): float32 CUDA input and parameters on x's device,
    sizes, and no autograd graph wanted (grad mode off, or neither x nor any parameter of the pass requires grad).
    ``training=True``: the plan of the trainable pass instead -- the same checks, but a graph must be wanted and the network
    must lie in the backward's range (``_hip.mlp_apply_bwd_supported``)."""
    return _fused_net.check_call(_KIND, match(net), x, n_samples, training)


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
        _fused_net.refuse_double_backward("MLPApplyFunction")
        x, w_in, b_in, s1, s2, u, b_mid, w_out, b_out = ctx.saved_tensors
        need = ctx.needs_input_grad
        gw_in, gw_mid, gw_out, gb, gx = _hip.mlp_apply_bwd(g, x, w_in, b_in, s1, s2, u, b_mid, w_out, mid_bias=ctx.mid_bias,
                                                          relu=ctx.relu, need_grad_x=need[0], act=ctx.act)
        n_mid, S, D = gw_mid.shape
        grad_x = gx.sum(dim=0) if gx is not None else None
        grad_b_in, grad_b_mid, grad_b_out = _fused_net.bias_grads(gb, n_mid, D, b_in, b_mid, b_out)
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


def _apply(x, w_in, b_in, s1, s2, u, b_mid, w_out, b_out, mid_bias, act_bits, act):
    return _hip.mlp_apply(x, w_in, b_in, s1, s2, u, b_mid, w_out, b_out, mid_bias=mid_bias, relu=act_bits, act=act)


def _stack(mids, drawn):
    """``s1, s2`` (n_mid, D) and ``u`` (n_mid, 1 + S, D) of the square layers; one layer: views, no copy launch."""
    if len(mids) == 1:
        return mids[0].s1.unsqueeze(0), mids[0].s2.unsqueeze(0), drawn[0][0].unsqueeze(0)
    return torch.stack([m.s1 for m in mids]), torch.stack([m.s2 for m in mids]), torch.stack([u for u, _ in drawn])


def run(net, p: Plan, x: torch.Tensor, n_samples: int, training: bool = False) -> torch.Tensor:
    """The pass (``_fused_net.launch``): each layer's draws in module order (``_mc_operands``, as ``forward_mc`` makes them),
    then ONE launch (``training``: through ``MLPApplyFunction``, for a plan of ``plan(..., training=True)``).  Returns
    ``(batch, 1, S)`` in forward_batched's layout; sets ``net._pass_kl`` like the batched route does."""
    y, drawn, (kl_in, kl_out) = _fused_net.launch(p, x, n_samples, _stack, MLPApplyFunction.apply if training else _apply)
    kls = [kl_in] + [kl for _, kl in drawn] + [kl_out]
    total = None
    if all(torch.is_tensor(k) for k in kls):
        for k in kls:
            total = k if total is None else total + k
    net._pass_kl = total
    return y
