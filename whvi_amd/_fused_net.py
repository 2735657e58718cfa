"""What the one-launch network passes share on the Python side: ``whvi_amd.fused_mlp`` (diagonal square layers) and
``whvi_amd.fused_fastfood`` (fastfood square layers) are this module plus what differs per kind of square layer.

Shared: the scan of the module list and the first / output layer checks behind ``match`` (``_scan``, ``_first_layer``,
``_output_layer``, ``_act_bits``), the checks of one call behind ``plan`` (``check_call``), the operand gathering and the launch
behind ``run`` (``launch``), and the two pieces every autograd Function's backward needs (``refuse_double_backward``,
``bias_grads``).  A ``Kind`` names what the shared code says and asks per kind.  Per kind stay: the square layers' type checks
and reasons, how their operands are stacked, the chain rule from the kernel's gradients to the parameters, and the KL bookkeeping."""
from typing import Callable, NamedTuple, Optional

import torch
import torch.nn as nn

from whvi_amd import _hip
from whvi_amd.layers import WHVILinear
from whvi_amd.weights import WHVIColumnMatrix, WHVIStackedMatrix


class Kind(NamedTuple):
    pass_name: str                   # "fused pass" / "fused fastfood pass": the predictive plan's refusal of a wanted graph
    bwd_range: str                   # "<square layers> is outside <entry point>'s range": the training plan's range refusal
    bwd_supported: Callable          # _hip.mlp_apply_bwd_supported / _hip.mlp_fastfood_apply_bwd_supported


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


def check_call(kind: Kind, p, x: torch.Tensor, n_samples: int, training: bool):
    """The checks of one call on ``p`` = ``match(net)`` (a reason is handed on): float32 CUDA input and parameters on x's device,
    sizes, and whether an autograd graph is wanted (grad mode on, and x or a parameter of the pass requires grad) -- the
    predictive plan refuses such a call, the training plan takes only such calls, within ``kind.bwd_supported``."""
    if isinstance(p, str):
        return p
    if x.device.type != "cuda" or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != p.n_in:
        return f"input: needs a float32 CUDA (batch, {p.n_in}) tensor"
    params = [t for m in p.layers for t in m.parameters()]
    if any(t.device != x.device or t.dtype != torch.float32 for t in params):
        return "parameters: float32 on the input's device only"
    S, B = int(n_samples), x.shape[0]
    if S < 1 or S * B >= 2 ** 32:
        return f"{S} samples x {B} rows: outside 1 .. 2^32 - 1 rows"
    wanted = torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in params))
    if not training:
        return f"an autograd graph is wanted (the {kind.pass_name} has no backward)" if wanted else p
    if not wanted:
        return "no autograd graph is wanted (the training pass is for passes that need one)"
    if not kind.bwd_supported(p.kind, len(p.mids), p.D):
        return f"hidden width {p.D} with {len(p.mids)} {kind.bwd_range}"
    return p


def _bias(w) -> Optional[torch.Tensor]:
    return None if w.bias is None else w.bias.reshape(-1)


def launch(p, x: torch.Tensor, n_samples: int, stack: Callable, apply: Callable):
    """The pass of plan ``p``: every layer's draws in module order -- ``_mc_operands`` of the first layer, of each square layer,
    of the output layer, as ``forward_mc`` makes them, which is what makes the pass bit-identical to the batched route -- then
    ``s1, s2, mid = stack(p.mids, drawn)`` and ONE launch, ``apply(x, w_in, b_in, s1, s2, mid, b_mid, w_out, b_out, mid_bias,
    act_bits, act)``.  Clears every layer's ``_mc_kl`` like forward_batched does.  Returns ``(y (batch, 1, S) in forward_batched's
    layout, what the square layers drew, the first and the output layer's KL)``."""
    S = int(n_samples)
    first = p.first
    w_in, kl_in = first._mc_operands(S)                             # (S, D, K) or (S, D)
    if p.kind == _hip.MLP_FIRST_COLUMN:
        xin = x
    else:
        xin = torch.zeros((x.shape[0], first.D_in), device=x.device)   # forward_mc's x_padded
        xin[:, :first.n_in] = x
    drawn = [w._mc_operands(S) for w in p.mids]
    w_out, kl_out = p.last._mc_operands(S)                          # (S, D)
    for m in p.layers:
        m._mc_kl = None
        m.weight_submodule._mc_kl = None
    s1, s2, mid = stack(p.mids, drawn)
    mid_bias = sum(1 << j for j, w in enumerate(p.mids) if w.bias is not None)
    b_mid = None
    if mid_bias:
        b_mid = torch.stack([w.bias.reshape(-1) if w.bias is not None else torch.zeros_like(w.s1) for w in p.mids])
    y = apply(xin, w_in, _bias(first), s1, s2, mid, b_mid, w_out, _bias(p.last), mid_bias, p.act_bits, p.act)
    return y.unsqueeze(-1).permute(1, 2, 0), drawn, (kl_in, kl_out)


def refuse_double_backward(name: str):
    if torch.is_grad_enabled():
        raise RuntimeError(f"{name}: the fused training pass has no double backward -- call backward() without "
                           "create_graph=True, or turn WHVINetwork.set_fused_training off for this pass")


def bias_grads(gb: torch.Tensor, n_mid: int, D: int, b_in, b_mid, b_out):
    """``(grad_b_in, grad_b_mid, grad_b_out)`` out of the kernels' ``grad_b`` ((1 + n_mid) D + 1: b_in, b_mid rows, b_out), each
    in its bias's shape, None for a bias the pass does not have."""
    return (gb[:D].view(b_in.shape) if b_in is not None else None,
            gb[D:(1 + n_mid) * D].view(b_mid.shape) if b_mid is not None else None,
            gb[(1 + n_mid) * D:].view(b_out.shape) if b_out is not None else None)
