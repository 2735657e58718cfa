"""Opt-in "fastfood" mode: the TEXTBOOK operator  x -> S1 . H . diag(g) . H . S2 . x  applied to activations.

NOT reference-equivalent, on purpose.  As written, the reference's weight construction scales ROWS between row
transforms and collapses to the diagonal matrix D diag(s1 g s2) (SURVEY.md finding 1); `WHVILinear` reproduces
that by default.  The paper's parameterisation (Rossi et al., the report's eq. for W = S1 H diag(g) H S2) is the
column-scaling pipeline the synthetic (batch, n_samples, D) kernel benchmarks exercise (BASELINE config 3).  This
module gives that pipeline -- `whvi_fused_shs_*` with `axis = COL`, include/whvi_hip.h -- a Module-level consumer:

    y[k] = s1 * fwht(g_k * fwht(s2 * x[k])),      g_k = g_mu + softplus(g_rho) * eps_k,   eps_k ~ N(0, I)

for every Monte-Carlo sample k in ONE launch, O(D log D) per row and without ever materialising a D x D weight
(the reference-equivalent path builds S matrices of D^2 floats and a batched GEMM).  Same parameter names, shapes,
initialisation and KL as `WHVISquarePow2Matrix` (src/weights.py:28-32, :52-64), so checkpoints interchange.

Parity: bit-exact against `oracle.pipeline(axis="col")` (compositions of the reference's own primitives --
`matmul_diag_right`, src/utils.py:15-23, and the C++ FWHT) and against the dense product with `build_H` in float64
(tests/test_fastfood.py).  Host tensors run the same ops through the host FWHT.

16-bit activations (opt-in, ``WHVIFastfoodMatrix.keep_half``): a float16 / bfloat16 CUDA input is by default promoted to
float32 by the first multiply and comes back as float32 through separate launches.  With ``keep_half = True`` the forward is
ONE launch of ``whvi_fused_shs_ex_f16 / _bf16`` -- float32 parameters, float32 arithmetic, one rounding when the row is
stored, 2 bytes read + 2 written per element -- and returns the input's dtype.  With ``fused_backward = True`` as well, a
backward that wants a parameter gradient is ONE launch of ``whvi_fused_shs_bwd_f16 / _bf16`` (6 bytes per element, float32
sums, ``grad_x`` rounded once) instead of two float32 upcasts and the float32 chain; both flags default to False.

Rectangular layers (``WHVIFastfoodStackedMatrix``, ``WHVILinear(..., mode="fastfood_stacked")``): the paper's stacking -- the
input zero-padded to ``D = 2^ceil(log2 n_in)``, ``J = ceil(n_out / D)`` independent square operators applied to it, their
outputs concatenated and the surplus columns dropped.  On the GPU the float32 forward is ONE launch of
``whvi_fused_shs_stacked_f32`` that reads a row once and writes all ``J`` blocks side by side, and with
``fused_backward = True`` the backward is ONE launch of ``whvi_fused_shs_stacked_bwd_f32``.  With
``fused_epilogue = True`` the bias, an ``nn.ReLU`` in front of / behind the layer (``WHVINetwork.forward_batched``) and the
narrowing to an ``n_out`` that is a multiple of 4 are part of that forward launch, ``whvi_fused_shs_stacked_layer_f32``, instead
of passes of their own over the ``(S, batch, J D)`` activations; all three flags default to False.  With
``keep_half = True`` a float16 / bfloat16 input takes ONE launch of ``whvi_fused_shs_stacked_f16 / _bf16`` over the same range
 and the output keeps its dtype; with ``fused_backward = True`` and ``fused_backward16 = True`` as well its backward
is ONE launch of ``whvi_fused_shs_stacked_bwd_f16 / _bf16`` (``grad_x`` rounded once instead of once per block and
once per add, which is why it is a flag of its own), per block otherwise; its epilogue is separate passes unless ``fused_epilogue = True`` and ``fused_epilogue16 = True`` fold it into
ONE launch of ``whvi_fused_shs_stacked_layer_f16 / _bf16`` (each element rounded once instead of up to three times,
hence a flag of its own; ``n_out`` a multiple of 8 for the folded narrowing).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from whvi_amd.utils import is_pow_of_2

__all__ = ["FastfoodFunction", "WHVIFastfoodMatrix", "FastfoodStackedFunction", "FastfoodStackedLayerFunction",
           "WHVIFastfoodStackedMatrix"]


def _fwht(x):
    """Row FWHT of a 2-D tensor on its own device: the HIP kernels or the native host library."""
    if x.device.type == "cuda":
        from whvi_amd import _hip
        return _hip.fwht_rows(x)
    import fwht_cpp
    return fwht_cpp.forward(x)


_HALF = (torch.float16, torch.bfloat16)


def _pipeline(x, a, b, c, n_samples, sample_stride, shared=False, keep_half=False):
    """a * fwht(b[s(r)] * fwht(c * x[r])) for every row r, s(r) = (r // sample_stride) % n_samples.  ``shared``: ``x`` holds
    ONE sample's rows (``sample_stride`` of them) and every sample reads them -- on the GPU straight from the caches
    (WHVI_FUSED_SRC_SHARED), elsewhere after expanding.  16-bit ``x`` takes the fused launch only with ``keep_half``
    (it has no shared-source form: the input is expanded); without it, it is promoted to float32 by ``c * x`` below."""
    if shared:
        if x.device.type == "cuda":
            from whvi_amd import _hip
            if _hip.fused_src_shared_supported(x.dtype, x.size(1)):
                # fwht(c * x) is the same for every sample: once, then ONE transform per sample on the shared result
                # (the same multiplies and butterflies in the same order as the two-transform launch: the same bits)
                t = _hip.fused_shs(x, None, c.reshape(1, -1), None, axis="col", n_samples=1, one_transform=True)
                return _hip.fused_shs(t, a, b, None, axis="col", n_samples=n_samples, sample_stride=sample_stride,
                                      src_shared=True, one_transform=True)
        x = x.repeat(n_samples, 1)
    if x.device.type == "cuda":
        from whvi_amd import _hip
        if _hip.fused_supported(x.dtype, x.size(1)) and (keep_half or x.dtype not in _HALF):
            return _hip.fused_shs(x, a, b, c, axis="col", n_samples=n_samples, sample_stride=sample_stride)
        # rows longer than one wavefront tile (D > 8192; f64 > 4096): the fused launch does not exist, the plain
        # transform does (a block per row and beyond) -- the same multiplies and butterflies as separate launches
    rows = torch.arange(x.size(0), device=x.device) // sample_stride % n_samples
    return a * _fwht(b[rows] * _fwht(c * x))


def _scale_fwht(x, vec, n_samples=1, sample_stride=1):
    """``fwht(vec[s(r)] * x[r])`` for every row -- ``vec`` of shape ``(D,)`` (shared) or ``(n_samples, D)`` with
    s(r) = (r // sample_stride) % n_samples -- as one launch of the fused kernel's one-transform form on the GPU."""
    per_sample = vec.dim() == 2
    if x.device.type == "cuda":
        from whvi_amd import _hip
        if _hip.fused_src_shared_supported(x.dtype, x.size(1)):
            return _hip.fused_shs(x, None, vec if per_sample else vec.reshape(1, -1), None, axis="col",
                                  n_samples=n_samples if per_sample else 1, sample_stride=sample_stride if per_sample else 1,
                                  one_transform=True)
    if per_sample:
        rows = torch.arange(x.size(0), device=x.device) // sample_stride % n_samples
        return _fwht(vec[rows] * x)
    return _fwht(vec * x)


def _fastfood_backward(grad_y, x, a, b, c, S, stride, shared, keep_half, fused_backward, needs):
    """``(grad_x, grad_a, grad_b, grad_c)`` of ``y = a * fwht(b_s * fwht(c * x))`` -- the backward of ``FastfoodFunction`` (its
    docstring describes the routes), also run per block by ``FastfoodStackedFunction``.  ``keep_half`` / ``fused_backward``: the
    flags as the forward resolved them; ``needs``: which of ``x, a, b, c`` want a gradient (the others come back as None)."""
    need_x, need_a, need_b, need_c = needs
    grad_y = grad_y.contiguous()
    grad_x = grad_a = grad_b = grad_c = None
    x_dtype = x.dtype
    if keep_half:
        if need_x and not (need_a or need_b or need_c or shared):
            return _pipeline(grad_y, c, b, a, S, stride, keep_half=True), None, None, None
        if (fused_backward and (need_a or need_b or need_c) and not (shared and need_x)
                and grad_y.dtype == x.dtype and grad_y.device == x.device
                and all(t.dtype == torch.float32 and t.device == x.device for t in (a, b, c))
                and grad_y.size(0) == S * stride):
            from whvi_amd import _hip
            if _hip.fused_shs_bwd16_supported(x.dtype, x.size(1)):
                # ONE 16-bit launch: no float32 copy of x or grad_y, the sums in float32 (a shared x wants no gradient here)
                grad_x, grad_a, grad_b, grad_c = _hip.fused_shs_bwd(grad_y, x, a, b, c, S, stride, shared=shared,
                                                                    need_x=need_x)
                return (grad_x, grad_a if need_a else None, grad_b.view_as(b) if need_b else None,
                        grad_c if need_c else None)
        x, grad_y = x.float(), grad_y.float()
    if (fused_backward and not keep_half and (need_a or need_b or need_c) and x.dtype == torch.float32 and grad_y.dtype == torch.float32
            and all(t.dtype == torch.float32 and t.device == x.device for t in (a, b, c))
            and grad_y.size(0) == S * stride):
        from whvi_amd import _hip
        if _hip.fused_shs_bwd_supported(torch.float32, x.size(1)):
            # ONE launch: t1, u, v, w stay in registers, the three sums leave the chip as one partial per block
            grad_x, grad_a, grad_b, grad_c = _hip.fused_shs_bwd(grad_y, x, a, b, c, S, stride, shared=shared,
                                                                need_x=need_x)
            if shared and grad_x is not None:
                grad_x = grad_x.view(S, stride, -1).sum(dim=0)
            return (grad_x, grad_a if need_a else None, grad_b.view_as(b) if need_b else None,
                    grad_c if need_c else None)
    if shared:
        # every sample read the same rows: their gradients add up (what autograd does for an expanded input)
        fold = lambda g: None if g is None else g.view(S, stride, -1).sum(dim=0)   # noqa: E731
        x = x.repeat(S, 1)
    else:
        fold = lambda g: g                                                        # noqa: E731
    if need_x and not (need_a or need_b or need_c):
        return fold(_pipeline(grad_y, c, b, a, S, stride)).to(x_dtype), None, None, None
    # Every transform of the backward pass is "scale, then FWHT" (optionally scaled again): ONE launch each through the
    # one-transform form of the fused kernel where it exists, the multiply + plain transform elsewhere -- the same
    # roundings either way (tests/test_streaming_parity_gpu.py pins the launch to multiply + fwht_rows bit for bit)
    t1 = _scale_fwht(x, c)                              # forward intermediate fwht(c * x), recomputed
    if need_a:
        grad_a = (grad_y * _scale_fwht(t1, b, S, stride)).sum(dim=0)
    v = _scale_fwht(grad_y, a)                          # gradient at (b * t1)
    if need_b:
        prod = v * t1
        if stride * S == x.size(0):                     # (S, rows_per_sample, D) layout: one segmented sum
            grad_b = prod.view(S, stride, -1).sum(dim=1)
        else:
            rows = torch.arange(x.size(0), device=x.device) // stride % S
            grad_b = torch.zeros_like(b).index_add_(0, rows, prod)
    if need_c or need_x:
        w = _scale_fwht(v, b, S, stride)                # gradient at (c * x)
        if need_c:
            grad_c = (w * x).sum(dim=0)
        if need_x:
            grad_x = fold(c * w).to(x_dtype)
    return grad_x, grad_a, grad_b, grad_c


class FastfoodFunction(torch.autograd.Function):
    """``y = a * fwht(b_s * fwht(c * x))`` on rows ``(n_samples, rows_per_sample, D)`` flattened, ``b``: (S, D).

    Forward: one fused launch.  The operator is linear in x and H is symmetric, so the gradient with respect to x is
    the same launch with a and c exchanged; the gradients of the three diagonals are products with the two
    intermediate transforms (recomputed, not stored) summed over rows.  First order only.

    ``keep_half`` (16-bit CUDA ``x`` that ``_hip.fused_supported`` covers, float32 ``a, b, c``): the forward is one 16-bit
    launch and returns ``x.dtype``; so is a backward that wants ``grad_x`` alone (``a`` and ``c`` exchanged).  A backward that
    wants a parameter gradient upcasts ``x`` and ``grad_y`` to float32 once -- 2 bytes read + 4 written per element each, and
    every pass behind them moves 4-byte elements -- runs the float32 code below, and returns float32 parameter gradients
    and ``grad_x`` cast to ``x.dtype``.

    ``fused_backward`` (float32 CUDA tensors, 64 <= D <= 4096, rows == n_samples * sample_stride, at least one of ``a, b, c``
    wanting a gradient): the backward is ONE launch of ``whvi_fused_shs_bwd_f32`` -- ``x`` and ``grad_y`` read once, ``grad_x``
    written once, no activation-sized temporary -- plus the sum over samples for a shared ``x``.  ``grad_x`` has the bits of
    the chain's; the parameter gradients are the same sums in another order.  Everything else -- host tensors,
    other dtypes or sizes, ``grad_x`` alone -- runs the code below unchanged.

    ``keep_half`` AND ``fused_backward`` (the ``keep_half`` conditions, float32 ``a, b, c`` on ``x``'s device, 64 <= D <= 4096,
    rows == n_samples * sample_stride, a parameter wanting a gradient): the backward is ONE launch of
    ``whvi_fused_shs_bwd_f16 / _bf16`` -- 6 * D bytes per row instead of the two upcasts and the float32 chain, no float32 copy
    of ``x`` or ``grad_y`` and no temporary but ``grad_x``.  ``grad_x`` is the 16-bit launch's (float32
    arithmetic, rounded once), the parameter gradients are float32.  A shared ``x`` takes the launch only when it wants no
    gradient: the per-sample gradients would each be rounded to 16 bits before they are added, where the chain rounds their
    float32 sum once, so that case keeps the chain."""

    @staticmethod
    def forward(ctx, x, a, b, c, n_samples, sample_stride, shared=False, keep_half=False, fused_backward=False):
        """``shared``: ``x`` is ``(sample_stride, D)``, the same rows for every sample (a layer's first Monte-Carlo pass on
        a ``(batch, D)`` input); the result still has ``n_samples * sample_stride`` rows.  ``fused_backward``: see the class."""
        ctx.fused_backward = bool(fused_backward) and x.device.type == "cuda"
        ctx.save_for_backward(x, a, b, c)
        ctx.n_samples, ctx.sample_stride, ctx.shared = int(n_samples), int(sample_stride), bool(shared)
        ctx.keep_half = bool(keep_half) and x.device.type == "cuda" and x.dtype in _HALF
        return _pipeline(x, a, b, c, ctx.n_samples, ctx.sample_stride, ctx.shared, ctx.keep_half)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, a, b, c = ctx.saved_tensors
        grads = _fastfood_backward(grad_y, x, a, b, c, ctx.n_samples, ctx.sample_stride, ctx.shared, ctx.keep_half,
                                   ctx.fused_backward, ctx.needs_input_grad[:4])
        return (*grads, None, None, None, None, None)


class WHVIFastfoodMatrix(nn.Module):
    """Square (D, D) WHVI layer in fastfood mode (see the module docstring): parameters ``s1, s2, g_mu, g_rho``
    (+ optional ``bias``) as in ``WHVISquarePow2Matrix``; ``forward(x)`` draws one eps, ``forward_mc(x, S)`` draws S
    and runs all samples in one launch."""
    fused_backward = False    # float32 CUDA activations (16-bit ones with keep_half), 64 <= D <= 4096: True = the backward is one launch (FastfoodFunction); False: the chain
    keep_half = False         # float16 / bfloat16 CUDA activations: True = one 16-bit launch, output in the input's dtype (False: promoted to float32)

    def __init__(self, D, lambda_=1e-5, bias=False):
        super().__init__()
        if not is_pow_of_2(D):
            raise ValueError("fastfood mode needs a power-of-two width")
        self.D, self.lambda_, self.padding = D, lambda_, 0
        # creation order = WHVISquarePow2Matrix's (bias, s1, s2, g_mu, g_rho): the same seed gives the same parameters
        self.bias = nn.Parameter(torch.zeros(1, D)) if bias else None
        self.s1 = nn.Parameter(torch.randn(D) * 0.01)
        self.s2 = nn.Parameter(torch.randn(D) * 0.01)
        self.g_mu = nn.Parameter(torch.zeros(D))
        self.g_rho = nn.Parameter(torch.rand(D) - 3)

    @property
    def g_sigma(self):
        return F.softplus(self.g_rho)

    @property
    def kl(self):
        from whvi_amd.weights import _posterior_kl
        return _posterior_kl(self.g_mu.unsqueeze(0), self.g_rho.unsqueeze(0), self.lambda_)

    def dense_weight(self, g):
        """The (D, D) matrix this layer applies for one g -- ``diag(s1) H diag(g) H diag(s2)`` -- built densely (tests,
        inspection; never used by forward)."""
        from whvi_amd.utils import build_H
        H = build_H(self.D, self.g_mu.device).to(self.g_mu.dtype)
        return self.s1.unsqueeze(1) * (H @ (g.unsqueeze(1) * (H * self.s2.unsqueeze(0))))

    def _mc_operands(self, n_samples):
        """g (S, D): every sample's diagonal for one batched pass -- row k from row k of one ``randn(n_samples, D)`` draw (the
        draw of ``forward_mc``; shared with the one-launch predictive pass, ``whvi_amd.fused_fastfood``)."""
        eps = torch.randn(n_samples, self.D, device=self.g_mu.device)
        return self.g_mu + self.g_sigma * eps

    def forward_mc(self, x, n_samples):
        """(batch, D) or (n_samples, batch, D) -> (n_samples, batch, D); sample k uses row k of one
        ``randn(n_samples, D)`` draw."""
        g = self._mc_operands(n_samples)                                          # (S, D)
        half = False
        if self.keep_half and x.device.type == "cuda" and x.dtype in _HALF and self.s1.dtype == torch.float32:
            from whvi_amd import _hip
            half = _hip.fused_supported(x.dtype, self.D)
        # (the bias is added in the activation's dtype)
        bias = None if self.bias is None else (self.bias.to(x.dtype) if half else self.bias)
        if x.dim() == 2:
            # a (batch, D) input shared by all samples: read by every sample straight from the caches, never expanded
            batch = x.size(0)
            out = FastfoodFunction.apply(x.contiguous(), self.s1, g, self.s2, n_samples, batch, True, half, self.fused_backward)
            out = out.view(n_samples, batch, self.D)
            return out + bias if bias is not None else out
        batch = x.size(1)
        rows = x.reshape(n_samples * batch, self.D).contiguous()
        out = FastfoodFunction.apply(rows, self.s1, g, self.s2, n_samples, batch, False, half,
                                     self.fused_backward).view(n_samples, batch, self.D)
        return out + bias if bias is not None else out

    def forward(self, x):
        out = self.forward_mc(x.reshape(-1, self.D), 1)[0].reshape(x.shape)
        return out


def _fastfood_stacked_backward(grad_y, x, a, b, c, S, stride, shared, keep_half, fused_backward, needs, fused_backward16=False):
    """``(grad_x, grad_a, grad_b, grad_c)`` of ``y[:, j * D:(j + 1) * D] = a[j] * fwht(b[j, s] * fwht(c[j] * x))`` -- the backward of
    ``FastfoodStackedFunction`` (its docstring describes the routes), also run by ``FastfoodStackedLayerFunction`` behind its
    masks.  ``keep_half`` / ``fused_backward`` / ``fused_backward16``: the flags as the forward resolved them; ``needs``: which
    of ``x, a, b, c`` want a gradient (the others come back as None)."""
    J, D = a.shape
    need_x, need_a, need_b, need_c = needs
    if (fused_backward and not keep_half and (need_a or need_b or need_c) and not (shared and need_x)
            and all(t.dtype == torch.float32 and t.device == x.device for t in (x, grad_y, a, b, c))
            and grad_y.size(0) == S * stride):
        from whvi_amd import _hip
        if _hip.fused_shs_stacked_bwd_supported(torch.float32, D, J):
            # ONE launch for all J blocks: x and the J segments of grad_y read once, grad_x written once.  (A shared x that
            # wants a gradient stays below: the launch adds the blocks per (sample, row) and the samples would be folded
            # afterwards, where the loop folds each block's samples first -- the same sum in another order, not the same bits.)
            grad_x, grad_a, grad_b, grad_c = _hip.fused_shs_stacked_bwd(grad_y, x, a, b, c, S, stride, shared=shared, need_x=need_x)
            return grad_x, grad_a if need_a else None, grad_b if need_b else None, grad_c if need_c else None
    if (keep_half and fused_backward and fused_backward16 and (need_a or need_b or need_c) and not (shared and need_x)
            and x.dtype in _HALF and grad_y.dtype == x.dtype and grad_y.device == x.device
            and all(t.dtype == torch.float32 and t.device == x.device for t in (a, b, c)) and grad_y.size(0) == S * stride):
        from whvi_amd import _hip
        if _hip.fused_shs_stacked_bwd16_supported(x.dtype, D, J):
            # ONE launch on the 16-bit streams: grad_x stays float32 across the blocks and is rounded once (the loop below rounds
            # each block's grad_x and each add: other bits, hence the flag).  (A shared x that wants a gradient stays below: the
            # per-sample 16-bit gradients would each be rounded before the fold over the samples.)
            grad_x, grad_a, grad_b, grad_c = _hip.fused_shs_stacked_bwd16(grad_y, x, a, b, c, S, stride, shared=shared, need_x=need_x)
            return grad_x, grad_a if need_a else None, grad_b if need_b else None, grad_c if need_c else None
    blocks = grad_y.view(grad_y.size(0), J, D)
    grad_x, per_block = None, []
    for j in range(J):
        gx, ga, gb, gc = _fastfood_backward(blocks[:, j].contiguous(), x, a[j], b[j], c[j], S, stride, shared, keep_half,
                                            fused_backward, (need_x, need_a, need_b, need_c))
        if gx is not None:
            grad_x = gx if grad_x is None else grad_x + gx
        per_block.append((ga, gb, gc))
    grad_a, grad_b, grad_c = (torch.stack([g[i] for g in per_block]) if need else None
                              for i, need in enumerate((need_a, need_b, need_c)))
    return grad_x, grad_a, grad_b, grad_c


class FastfoodStackedFunction(torch.autograd.Function):
    """``y[:, j * D:(j + 1) * D] = a[j] * fwht(b[j, s] * fwht(c[j] * x))`` for ``j = 0 .. J - 1``: ``J`` square fastfood operators
    on the same rows ``(n_samples, rows_per_sample, D)`` flattened, side by side.  ``a, c``: (J, D); ``b``: (J, S, D).

    Forward: ONE launch of ``whvi_fused_shs_stacked_f32`` for float32 CUDA tensors that ``_hip.fused_shs_stacked_supported``
    covers -- the row read once, ``J`` segments written -- and otherwise (host tensors, other dtypes, D < 64 or D > 2048, more
    blocks than fit the launch's LDS) the concatenation of ``FastfoodFunction``'s forward per block, which block ``j`` of the
    launch equals bit for bit.  ``keep_half`` (float16 / bfloat16 CUDA ``x``, float32 ``a, b, c`` on its device, a ``(D, J)`` that
    ``_hip.fused_shs_stacked16_supported`` covers -- the float32 launch's range): ONE launch of ``whvi_fused_shs_stacked_f16 /
    _bf16``, the output in ``x``'s dtype and block ``j`` the bits of ``FastfoodFunction``'s 16-bit forward; outside
    that range the per-block 16-bit launches and their concatenation.  Backward (unless a paragraph below applies): per block, what ``FastfoodFunction.backward`` runs on that block's columns of
    ``grad_y`` (``keep_half`` and ``fused_backward`` as there); the blocks' ``grad_x`` add up.  First order only.

    ``fused_backward`` without ``keep_half`` (float32 tensors on ``x``'s device, rows == n_samples * sample_stride, at least one
    of ``a, b, c`` wanting a gradient, 2 <= J <= 4 for 64 <= D <= 1024 or J = 2 at D = 2048 --
    ``_hip.fused_shs_stacked_bwd_supported``): the backward is ONE launch of ``whvi_fused_shs_stacked_bwd_f32`` for all blocks
    -- ``x`` and the ``J`` segments of ``grad_y`` read once, ``grad_x`` written once, no copy of a segment, no per-block
    ``grad_x`` and no running sum.  Every gradient has the bits of the per-block loop with the flag set.  A shared
    ``x`` that wants a gradient keeps the loop (the launch adds the blocks before the samples, the loop the samples before the
    blocks); so does everything else -- ``J = 1``, ``J > 4``, D = 4096, host tensors, other dtypes, the flag off.

    ``keep_half`` AND ``fused_backward`` AND ``fused_backward16`` (16-bit ``x`` and ``grad_y`` of one dtype, float32 ``a, b, c`` on
    ``x``'s device, rows == n_samples * sample_stride, at least one of ``a, b, c`` wanting a gradient, ``x`` not a shared input
    that itself wants a gradient, a ``(D, J)`` that ``_hip.fused_shs_stacked_bwd16_supported`` covers -- the float32 launch's
    range): the backward is ONE launch of ``whvi_fused_shs_stacked_bwd_f16 / _bf16``.  The parameter gradients
    have the bits of the per-block 16-bit launches; ``grad_x`` is accumulated in float32 and rounded ONCE, where the loop rounds
    ``2 J - 1`` times, so its bits differ (it is the closer one) -- which is why this is a flag of its own.  Everything else
    runs what it runs without the flag."""

    @staticmethod
    def forward(ctx, x, a, b, c, n_samples, sample_stride, shared=False, keep_half=False, fused_backward=False,
                fused_backward16=False):
        ctx.fused_backward = bool(fused_backward) and x.device.type == "cuda"
        ctx.fused_backward16 = bool(fused_backward16) and x.device.type == "cuda"
        ctx.save_for_backward(x, a, b, c)
        ctx.n_samples, ctx.sample_stride, ctx.shared = int(n_samples), int(sample_stride), bool(shared)
        ctx.keep_half = bool(keep_half) and x.device.type == "cuda" and x.dtype in _HALF
        if x.device.type == "cuda" and all(t.dtype == torch.float32 and t.device == x.device for t in (x, a, b, c)):
            from whvi_amd import _hip
            if _hip.fused_shs_stacked_supported(torch.float32, x.size(1), a.size(0)):
                return _hip.fused_shs_stacked(x, a, b, c, ctx.n_samples, ctx.sample_stride, shared=ctx.shared)
        if ctx.keep_half and all(t.dtype == torch.float32 and t.device == x.device for t in (a, b, c)):
            from whvi_amd import _hip
            if _hip.fused_shs_stacked16_supported(x.dtype, x.size(1), a.size(0)):
                # 16-bit activations: ONE launch as well, each block's bits those of its 16-bit launch below
                return _hip.fused_shs_stacked16(x, a, b, c, ctx.n_samples, ctx.sample_stride, shared=ctx.shared)
        return torch.cat([_pipeline(x, a[j], b[j], c[j], ctx.n_samples, ctx.sample_stride, ctx.shared, ctx.keep_half)
                          for j in range(a.size(0))], dim=1)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, a, b, c = ctx.saved_tensors
        grads = _fastfood_stacked_backward(grad_y, x, a, b, c, ctx.n_samples, ctx.sample_stride, ctx.shared, ctx.keep_half,
                                           ctx.fused_backward, ctx.needs_input_grad[:4], fused_backward16=ctx.fused_backward16)
        return (*grads, None, None, None, None, None, None)


class FastfoodStackedLayerFunction(torch.autograd.Function):
    """``y = act_out(FastfoodStackedFunction(act_in(x), a, b, c) + bias)[:, :n_cols]`` in ONE launch of
    ``whvi_fused_shs_stacked_layer_f32``: float32 CUDA tensors that ``_hip.fused_shs_stacked_layer_supported``
    covers, ``bias`` of ``J * D`` elements or None, ``n_cols`` a multiple of 4 in ``((J - 1) D, J D]``, ``act_in`` / ``act_out``
    ``torch.relu`` with ``relu_in`` / ``relu_out``.  The values are those of the separate passes, bit for bit.

    Backward: composed from what exists -- the mask of ``relu_out`` from the saved output (saved only then), the bias gradient
    as the row sum, the gradient zero-padded to ``J * D`` columns, ``act_in(x)`` recomputed, ``FastfoodStackedFunction``'s
    backward (``fused_backward`` as there), and the mask of ``relu_in`` on ``grad_x``: the same operands in the same launches as
    the separate passes' autograd graph.  First order only.

    ``fused_epilogue_backward`` AND ``fused_backward`` (float32 tensors on one CUDA device, rows == n_samples * sample_stride, at
    least one of ``a, b, c, bias`` wanting a gradient, ``x`` not a shared input that itself wants a gradient, a ``(D, J, bias)``
    that ``_hip.fused_shs_stacked_layer_bwd_supported`` covers, and a mask or a padding to fold -- ``relu_in``, ``relu_out`` or
    ``n_cols < J * D``; with nothing but the bias sum the launch measured no faster than the row sum and the launch it starts
    from, so that case stays composed): the backward is ONE launch of
    ``whvi_fused_shs_stacked_layer_bwd_f32`` -- both masks, the zero padding and the bias sum inside it, so the
    masked gradient, its padded copy, ``act_in(x)`` and the unmasked ``grad_x`` are never materialised.  ``grad_x`` and the
    gradients of ``a, b, c`` have the bits of the composed backward with ``fused_backward`` set; the bias gradient is the same
    sum in another (deterministic) order, which is why this is a flag of its own.  Everything else runs the composed backward."""

    @staticmethod
    def forward(ctx, x, a, b, c, bias, n_cols, relu_in, relu_out, n_samples, sample_stride, shared=False, fused_backward=False,
                fused_epilogue_backward=False):
        from whvi_amd import _hip
        ctx.n_samples, ctx.sample_stride, ctx.shared = int(n_samples), int(sample_stride), bool(shared)
        ctx.relu_in, ctx.relu_out, ctx.fused_backward = bool(relu_in), bool(relu_out), bool(fused_backward)
        ctx.fused_epilogue_backward = bool(fused_epilogue_backward)
        y = _hip.fused_shs_stacked_layer(x, a, b, c, ctx.n_samples, ctx.sample_stride, bias=bias, n_cols=n_cols, relu_in=ctx.relu_in,
                                         relu_out=ctx.relu_out, shared=ctx.shared)
        ctx.bias_shape = None if bias is None else bias.shape
        ctx.save_for_backward(x, a, b, c, y if ctx.relu_out else None)     # (the activation's mask comes from its own output)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, a, b, c, y = ctx.saved_tensors
        full = a.numel()                                                   # J * D
        need_x, need_a, need_b, need_c, need_bias = ctx.needs_input_grad[:5]
        need_bias = need_bias and ctx.bias_shape is not None
        S, stride = ctx.n_samples, ctx.sample_stride
        # a mask or the padding to fold: with the bias sum alone the launch measured no faster
        folds = ctx.relu_in or ctx.relu_out or grad_y.size(1) < full
        if (ctx.fused_epilogue_backward and ctx.fused_backward and folds and (need_a or need_b or need_c or need_bias)
                and not (ctx.shared and need_x) and grad_y.size(0) == S * stride
                and all(t.dtype == torch.float32 and t.device == x.device and t.device.type == "cuda"
                        for t in (x, grad_y, a, b, c) + ((y,) if ctx.relu_out else ()))):
            from whvi_amd import _hip
            if _hip.fused_shs_stacked_layer_bwd_supported(torch.float32, a.size(1), a.size(0), need_bias):
                # ONE launch: the masks, the padding and the bias sum inside it (a shared x that wants a gradient stays
                # below for _fastfood_stacked_backward's reason)
                if ctx.relu_out and grad_y.size(0) > 1 and grad_y.stride(0) != y.stride(0):
                    grad_y = grad_y.contiguous()       # (a view of a wider gradient, e.g. behind torch.cat: y's pitch is n_cols)
                grad_x, grad_a, grad_b, grad_c, grad_bias = _hip.fused_shs_stacked_layer_bwd(
                    grad_y, y, x, a, b, c, S, stride, n_cols=grad_y.size(1), relu_in=ctx.relu_in, relu_out=ctx.relu_out,
                    shared=ctx.shared, need_x=need_x, need_bias=need_bias)
                return (grad_x, grad_a if need_a else None, grad_b if need_b else None, grad_c if need_c else None,
                        grad_bias.view(ctx.bias_shape) if need_bias else None, None, None, None, None, None, None, None, None)
        g = (torch.ops.aten.threshold_backward(grad_y, y, 0) if ctx.relu_out else grad_y).contiguous()
        grad_bias = None
        if ctx.bias_shape is not None and ctx.needs_input_grad[4]:
            grad_bias = F.pad(g.sum(dim=0), (0, full - g.size(1))).view(ctx.bias_shape)
        if g.size(1) < full:
            g = F.pad(g, (0, full - g.size(1)))
        xin = torch.relu(x) if ctx.relu_in else x
        grad_x, grad_a, grad_b, grad_c = _fastfood_stacked_backward(g, xin, a, b, c, ctx.n_samples, ctx.sample_stride, ctx.shared,
                                                                    False, ctx.fused_backward, ctx.needs_input_grad[:4])
        if ctx.relu_in and grad_x is not None:
            grad_x = torch.ops.aten.threshold_backward(grad_x, xin, 0)
        return grad_x, grad_a, grad_b, grad_c, grad_bias, None, None, None, None, None, None, None, None


def _layer_bwd16_pays(d, n_blocks, n_samples, sample_stride, n_cols, relu_out, shared, need_x, need_bias):
    """Routing of ``FastfoodStackedLayer16Function.backward`` by measurement: False where the one launch measured
    slower than the composed backward -- four blocks with the bias sum (one wave per SIMD where the composed route's launch runs
    two) or D = 2048, on a grid of more than 256 blocks (more than one per CU) whose bytes stay in the Infinity Cache (at most
    256 MiB: the launch's own streaming rule).  Smaller grids and streaming launches measured faster at every such ``(D, J)``."""
    if not ((n_blocks == 4 and need_bias) or d == 2048):
        return True
    rows = n_samples * sample_stride
    if rows * 2 * (n_cols * (2 if relu_out else 1) + (0 if shared else d) + (d if need_x else 0)) > (256 << 20):
        return True
    from whvi_amd import _hip
    slot = (16 if need_bias else 12) * d * n_blocks          # bytes of one block's slot: the workspace query counts the grid
    blocks = int(_hip.lib().whvi_fused_shs_stacked_layer_bwd_workspace(n_samples, sample_stride, d.bit_length() - 1, n_blocks,
                                                                      1 if need_bias else 0)) // slot
    return blocks <= 256


class FastfoodStackedLayer16Function(torch.autograd.Function):
    """``FastfoodStackedLayerFunction`` on 16-bit activations: ``y = act_out(stacked(act_in(x), a, b, c) + bias)[:, :n_cols]`` in
    ONE launch of ``whvi_fused_shs_stacked_layer_f16 / _bf16`` -- float16 / bfloat16 CUDA ``x``, float32 ``a, b, c``
    and ``bias`` (``J * D`` elements or None) on its device, a ``(D, J, bias)`` that ``_hip.fused_shs_stacked_layer16_supported``
    covers, ``n_cols`` a multiple of 8 in ``((J - 1) D, J D]``.  The arithmetic is float32 on the exactly-upcast input and every
    element is rounded to 16 bits ONCE, where the separate passes (the 16-bit launch, ``+ bias.to(dtype)``, ``torch.relu``) round
    up to three times: the values are the closer ones, not the same bits.

    Backward: composed from what exists -- the mask of ``relu_out`` from the saved output (saved only then), the bias gradient
    as the float32 row sum of the masked 16-bit gradient, the gradient zero-padded to ``J * D`` columns, ``act_in(x)``
    recomputed, ``FastfoodStackedFunction``'s 16-bit backward (``fused_backward`` / ``fused_backward16`` as there), and the mask
    of ``relu_in`` on ``grad_x``.  First order only.

    ``fused_epilogue_backward16`` AND ``fused_backward`` AND ``fused_backward16`` (16-bit ``x`` and ``grad_y`` of one dtype on a CUDA
    device, float32 ``a, b, c`` and ``bias`` on it, rows == n_samples * sample_stride, at least one of ``a, b, c, bias`` wanting a
    gradient, ``x`` not a shared input that itself wants a gradient, a ``(D, J, bias)`` that
    ``_hip.fused_shs_stacked_layer_bwd16_supported`` covers, and a mask or a padding to fold -- ``relu_in``, ``relu_out`` or
    ``n_cols < J * D``; with nothing but the bias sum the case stays composed, as in float32 -- and not one of the cached,
    full-grid cases that measured slower, ``_layer_bwd16_pays``): the backward is ONE launch of
    ``whvi_fused_shs_stacked_layer_bwd_f16 / _bf16`` -- both masks, the zero padding and the bias sum inside it, so
    the masked gradient, its padded copy, ``act_in(x)`` and the unmasked ``grad_x`` are never materialised.  ``grad_x`` and the
    gradients of ``a, b, c`` have the bits of the composed backward with both backward flags set; the bias gradient is the same
    float32 sum in another (deterministic) order, which is why this is a flag of its own.  Everything else runs the composed
    backward."""

    @staticmethod
    def forward(ctx, x, a, b, c, bias, n_cols, relu_in, relu_out, n_samples, sample_stride, shared=False, fused_backward=False,
                fused_backward16=False, fused_epilogue_backward16=False):
        from whvi_amd import _hip
        ctx.n_samples, ctx.sample_stride, ctx.shared = int(n_samples), int(sample_stride), bool(shared)
        ctx.relu_in, ctx.relu_out = bool(relu_in), bool(relu_out)
        ctx.fused_backward, ctx.fused_backward16 = bool(fused_backward), bool(fused_backward16)
        ctx.fused_epilogue_backward16 = bool(fused_epilogue_backward16)
        ctx.bias_f32 = bias is None or (bias.dtype == torch.float32 and bias.device == x.device)
        y = _hip.fused_shs_stacked_layer16(x, a, b, c, ctx.n_samples, ctx.sample_stride, bias=bias, n_cols=n_cols,
                                           relu_in=ctx.relu_in, relu_out=ctx.relu_out, shared=ctx.shared)
        ctx.bias_shape = None if bias is None else bias.shape
        ctx.save_for_backward(x, a, b, c, y if ctx.relu_out else None)     # (the activation's mask comes from its own output)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, a, b, c, y = ctx.saved_tensors
        full = a.numel()                                                   # J * D
        need_x, need_a, need_b, need_c, need_bias = ctx.needs_input_grad[:5]
        need_bias = need_bias and ctx.bias_shape is not None
        S, stride = ctx.n_samples, ctx.sample_stride
        # a mask or the padding to fold: with the bias sum alone the case stays composed
        folds = ctx.relu_in or ctx.relu_out or grad_y.size(1) < full
        if (ctx.fused_epilogue_backward16 and ctx.fused_backward and ctx.fused_backward16 and folds
                and (need_a or need_b or need_c or need_bias) and not (ctx.shared and need_x) and grad_y.size(0) == S * stride
                and x.device.type == "cuda" and x.dtype in _HALF and grad_y.dtype == x.dtype and grad_y.device == x.device
                and ctx.bias_f32 and all(t.dtype == torch.float32 and t.device == x.device for t in (a, b, c))):
            from whvi_amd import _hip
            if (_hip.fused_shs_stacked_layer_bwd16_supported(x.dtype, a.size(1), a.size(0), need_bias)
                    and _layer_bwd16_pays(a.size(1), a.size(0), S, stride, grad_y.size(1), ctx.relu_out, ctx.shared, need_x,
                                          need_bias)):
                # ONE launch: the masks, the padding and the bias sum inside it (a shared x that wants a gradient stays
                # below for _fastfood_stacked_backward's reason)
                if ctx.relu_out and grad_y.size(0) > 1 and grad_y.stride(0) != y.stride(0):
                    grad_y = grad_y.contiguous()       # (a view of a wider gradient, e.g. behind torch.cat: y's pitch is n_cols)
                grad_x, grad_a, grad_b, grad_c, grad_bias = _hip.fused_shs_stacked_layer_bwd16(
                    grad_y, y, x, a, b, c, S, stride, n_cols=grad_y.size(1), relu_in=ctx.relu_in, relu_out=ctx.relu_out,
                    shared=ctx.shared, need_x=need_x, need_bias=need_bias)
                return (grad_x, grad_a if need_a else None, grad_b if need_b else None, grad_c if need_c else None,
                        grad_bias.view(ctx.bias_shape) if need_bias else None, None, None, None, None, None, None, None, None, None)
        g = (torch.ops.aten.threshold_backward(grad_y, y, 0) if ctx.relu_out else grad_y).contiguous()
        grad_bias = None
        if ctx.bias_shape is not None and ctx.needs_input_grad[4]:
            grad_bias = F.pad(g.sum(dim=0, dtype=torch.float32), (0, full - g.size(1))).view(ctx.bias_shape)
        if g.size(1) < full:
            g = F.pad(g, (0, full - g.size(1)))
        xin = torch.relu(x) if ctx.relu_in else x
        grad_x, grad_a, grad_b, grad_c = _fastfood_stacked_backward(g, xin, a, b, c, ctx.n_samples, ctx.sample_stride, ctx.shared,
                                                                    True, ctx.fused_backward, ctx.needs_input_grad[:4],
                                                                    ctx.fused_backward16)
        if ctx.relu_in and grad_x is not None:
            grad_x = torch.ops.aten.threshold_backward(grad_x, xin, 0)
        return grad_x, grad_a, grad_b, grad_c, grad_bias, None, None, None, None, None, None, None, None, None


class WHVIFastfoodStackedMatrix(nn.Module):
    """Rectangular (n_out, n_in) WHVI layer in fastfood mode: ``stack`` square ``WHVIFastfoodMatrix`` blocks of width
    ``D_in = 2^ceil(log2 n_in)`` applied to the zero-padded input, their outputs concatenated and narrowed to ``n_out``
    (dimensions: ``WHVIStackedMatrix.setup_dimensions``).  Parameters ``weight_matrices.<j>.{s1, s2, g_mu, g_rho}`` (+ optional
    ``bias`` (1, D_out)) -- the checkpoint keys and the creation order of ``WHVIStackedMatrix``, so its state dict loads and the
    same seed gives the same parameters.  The flags below choose the launches (all default to False; ``FastfoodStackedFunction``
    and ``FastfoodStackedLayerFunction`` describe the routes): on float16 / bfloat16 activations ``keep_half`` keeps them 16-bit
    through one forward launch, and with ``fused_backward`` and ``fused_backward16`` as well the backward of all blocks is one
    16-bit launch that rounds ``grad_x`` once."""
    fused_backward = False    # True = the backward of all blocks is one launch (float32, 2 .. 4 blocks of 64 <= D_in <= 1024, 2 of 2048: FastfoodStackedFunction), elsewhere each block's is one launch where FastfoodFunction's is
    keep_half = False         # as on WHVIFastfoodMatrix: 16-bit CUDA activations stay 16-bit (forward: one launch for all blocks where _hip.fused_shs_stacked16_supported, per-block launches elsewhere; backward: per block, or one launch with fused_backward16; the epilogue is separate passes unless fused_epilogue16 folds it)
    fused_backward16 = False  # True (with keep_half and fused_backward) = the 16-bit backward of all blocks is one launch (where _hip.fused_shs_stacked_bwd16_supported: FastfoodStackedFunction); grad_x is rounded once instead of 2 J - 1 times, so its bits differ from the per-block route's; the parameter gradients are bit-equal
    fused_epilogue = False    # True = the bias, the neighbouring nn.ReLUs and the narrowing to n_out (a multiple of 4) are folded into the forward launch (float32, where _hip.fused_shs_stacked_layer_supported: FastfoodStackedLayerFunction)
    fused_epilogue16 = False  # True (with keep_half and fused_epilogue) = on float16 / bfloat16 CUDA activations the bias, the neighbouring nn.ReLUs and the narrowing to n_out (a multiple of 8) are folded into the 16-bit forward launch (where _hip.fused_shs_stacked_layer16_supported: FastfoodStackedLayer16Function); each element is rounded once instead of up to three times, so its bits differ from the separate passes'
    fused_epilogue_backward = False    # True (with fused_backward and fused_epilogue) = the backward of that launch is one launch too, with both masks and the bias sum folded in (float32, where _hip.fused_shs_stacked_layer_bwd_supported and a ReLU or a narrowing is folded); the bias gradient's bits differ from the composed backward's (another summation order), all other gradients are bit-equal
    fused_epilogue_backward16 = False  # True (with keep_half, fused_epilogue, fused_epilogue16, fused_backward and fused_backward16) = the backward of the 16-bit epilogue launch is one launch too, with both masks and the bias sum folded in (float16 / bfloat16, where _hip.fused_shs_stacked_layer_bwd16_supported and a ReLU or a narrowing is folded; four blocks with the bias sum, or D_in = 2048, on a full grid of cached bytes stay composed, _layer_bwd16_pays); the bias gradient's bits differ from the composed backward's (another summation order), all other gradients are bit-equal

    def __init__(self, n_in, n_out, lambda_=1e-5, bias=False):
        super().__init__()
        from whvi_amd.weights import WHVIStackedMatrix
        self.n_in, self.n_out, self.lambda_ = n_in, n_out, lambda_
        self.D_in, self.D_out, self.padding, self.stack = WHVIStackedMatrix.setup_dimensions(n_in, n_out)
        self.weight_matrices = nn.ModuleList([WHVIFastfoodMatrix(self.D_in, lambda_=lambda_) for _ in range(self.stack)])
        self.bias = nn.Parameter(torch.zeros(1, self.D_out)) if bias else None

    @property
    def kl(self):
        return sum(m.kl for m in self.weight_matrices)

    def _stacked(self, name):
        """(stack, D_in) tensor of one per-block vector."""
        return torch.stack([getattr(m, name) for m in self.weight_matrices])

    def fuses_relu(self, x):
        """True when ``forward_mc(x, ..., relu_in=, relu_out=)`` folds the activations (and the bias and the narrowing) into its
        one launch: ``fused_epilogue`` set, float32 ``x`` and parameters on one CUDA device (so ``keep_half`` does not apply) and
        a ``(D_in, stack, bias)`` the launch covers.  Otherwise they are separate ``torch.relu`` passes -- same values either way.
        With ``fused_epilogue16`` AND ``keep_half`` as well, also for a float16 / bfloat16 ``x`` (float32 parameters on its device,
        a ``(D_in, stack, bias)`` that ``_hip.fused_shs_stacked_layer16_supported`` covers): the 16-bit launch rounds once where
        the separate passes round up to three times -- the closer values, not the same bits."""
        if not self.fused_epilogue or x.device.type != "cuda":
            return False
        half = x.dtype in _HALF and self.fused_epilogue16 and self.keep_half
        if x.dtype != torch.float32 and not half:
            return False
        if any(p.dtype != torch.float32 or p.device != x.device for p in self.parameters()):
            return False
        from whvi_amd import _hip
        if half:
            return _hip.fused_shs_stacked_layer16_supported(x.dtype, self.D_in, self.stack, self.bias is not None)
        return _hip.fused_shs_stacked_layer_supported(torch.float32, self.D_in, self.stack, self.bias is not None)

    def forward_mc(self, x, n_samples, relu_in=False, relu_out=False):
        """(batch, n_in) or (n_samples, batch, n_in) -> (n_samples, batch, n_out); sample k of block j uses row ``[j, k]`` of
        one ``randn(stack, n_samples, D_in)`` draw.  ``relu_in`` / ``relu_out``: ``relu(layer(relu(x)))``, folded into the launch
        where ``fuses_relu(x)``."""
        fold = self.fuses_relu(x)
        if (relu_in or relu_out) and not fold:
            out = self.forward_mc(torch.relu(x) if relu_in else x, n_samples)
            return torch.relu(out) if relu_out else out
        s1, s2, g_mu = self._stacked("s1"), self._stacked("s2"), self._stacked("g_mu")
        eps = torch.randn(self.stack, n_samples, self.D_in, device=g_mu.device)
        g = g_mu.unsqueeze(1) + F.softplus(self._stacked("g_rho")).unsqueeze(1) * eps                 # (J, S, D)
        if self.padding > 0:
            x = F.pad(x, (0, self.padding))
        half = False
        if self.keep_half and x.device.type == "cuda" and x.dtype in _HALF and s1.dtype == torch.float32:
            from whvi_amd import _hip
            half = _hip.fused_supported(x.dtype, self.D_in)
        shared = x.dim() == 2                  # a (batch, D) input shared by all samples: read by every sample, never expanded
        batch = x.size(0) if shared else x.size(1)
        rows = x.contiguous() if shared else x.reshape(n_samples * batch, self.D_in).contiguous()
        if fold and x.dtype in _HALF:
            # 16-bit activations (fused_epilogue16): a chunk holds 8 columns, so the narrowing is folded where n_out % 8 == 0
            narrow = self.n_out < self.D_out and self.n_out % 8 == 0
            if self.bias is not None or relu_in or relu_out or narrow:
                n_cols = self.n_out if narrow else self.D_out
                out = FastfoodStackedLayer16Function.apply(rows, s1, g, s2, self.bias, n_cols, relu_in, relu_out, n_samples, batch,
                                                           shared, self.fused_backward, self.fused_backward16,
                                                           self.fused_epilogue_backward16)
                out = out.view(n_samples, batch, n_cols)
                return out if n_cols == self.n_out else out[..., :self.n_out]
            fold = False                       # nothing to fold: the plain 16-bit launch below
        narrow = self.n_out < self.D_out and self.n_out % 4 == 0
        if fold and (self.bias is not None or relu_in or relu_out or narrow):
            # ONE launch with the epilogue: no pass for the bias, none for a ReLU, and n_out columns written at pitch n_out where
            # that is a multiple of 4 (otherwise pitch D_out and the narrowing view, as below)
            n_cols = self.n_out if self.n_out % 4 == 0 else self.D_out
            out = FastfoodStackedLayerFunction.apply(rows, s1, g, s2, self.bias, n_cols, relu_in, relu_out, n_samples, batch, shared,
                                                     self.fused_backward, self.fused_epilogue_backward).view(n_samples, batch, n_cols)
            return out if n_cols == self.n_out else out[..., :self.n_out]
        out = FastfoodStackedFunction.apply(rows, s1, g, s2, n_samples, batch, shared, half, self.fused_backward,
                                            self.fused_backward16)
        out = out.view(n_samples, batch, self.D_out)        # (the launch always writes pitch D_out)
        if self.bias is not None:
            out = out + (self.bias.to(x.dtype) if half else self.bias)
        return out[..., :self.n_out]

    def forward(self, x):
        return self.forward_mc(x.reshape(-1, self.n_in), 1)[0].reshape(*x.shape[:-1], self.n_out)
