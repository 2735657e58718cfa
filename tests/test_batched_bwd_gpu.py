"""The batched training route's backward at streaming sizes, config 4's share (16 samples x 45 730 rows, D = 1024) included:
whvi_diag_apply_bwd (whvi_amd/csrc/diag_apply.hpp) on each of its three code paths, and the torch-op backwards of the layers
around it (SmallKApplyFunction, RowDotFunction in whvi_amd/weights.py).

(a) The bwd kernel's summation order depends on (sample, slab) alone -- a slab's rows serially in a fixed order, the slabs in
    a fixed order in the finishing kernel -- and its paths differ only in block order and cache policy: the cached launch, the
    NT launch (non-temporal loads, beyond NT_MIN_BYTES = 256 MiB) and the long-stream launch (XCD-contiguous block order and
    write-through `sc1 nt` inline-asm stores of grad_x, from 4 GiB of streamed bytes up).  So every path gives the same bits.
(b) grad_x is ONE rounding of g * w_k: bit for bit the product of torch ops with the ReLU masks recomputed the way the kernel
    does; the four slots of `out` are float64 sums of the same float32 operands within 1e-5 of A64 (the float64 sum of the
    terms' absolute values), the bound of tests/test_mlp_train_gpu.py.
(c) The torch-op backwards at config 4's lengths, on the operands the config-4 network produces, within the same bound.
(d) Every launch here writes into buffers with sentinel margins and sentinel contents: no byte outside them may change and
    every output element must be written (a lost store cannot hide behind a stale value of an earlier call)."""
import os
import sys

import pytest
import torch

from whvi_amd import _hip
from whvi_amd.weights import DiagApplyFunction, RowDotFunction, SmallKApplyFunction

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mlp_train_gpu import _operands as _net_operands  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GiB = 1 << 30
NT_MIN_BYTES = 256 << 20          # dispatch.hpp: NT loads beyond this many streamed bytes
LONG_STREAM_BYTES = 4 << 30       # diag_apply_bwd_dispatch: XCD order + write-through stores from this many up
PAD = 4096                        # sentinel elements in front of and behind every output buffer
SENT = {torch.float32: -7.25e33, torch.float64: -7.25e303}
PATHS = {"default": 0, "cached": _hip.DIAG_TUNE_CACHED, "nt": _hip.DIAG_TUNE_NT,
         "nt plain order": _hip.DIAG_TUNE_NT | _hip.DIAG_TUNE_PLAIN_ORDER}


# ---- (a) / (b) / (d): whvi_diag_apply_bwd
# name, dtype, D, S, B, shared x, mean_plus, bias, relu_in, relu_out, need_grad_x, poisoned rows
CASES = [
    # config 4's share: 3 x 3.0 GB streamed (g, x read, grad_x written) = 9.0 GB >= 4 GiB: long stream; 128 slabs x 16
    # samples = 2048 blocks, a multiple of 8: XCD-contiguous order on
    ("config4_share", torch.float32, 1024, 16, 45730, False, True, True, False, True, True, 0),
    # 3 x 1.43 GB = 4.30 GB >= 4 GiB: long stream; 293 slabs x 7 samples = 2051 blocks: the reorder is off
    ("long_odd_grid", torch.float32, 1024, 7, 50000, False, False, False, True, False, True, 0),
    # 3 x 0.66 GB = 1.97 GB: between 256 MiB and 4 GiB, the NT path
    ("nt_midsize", torch.float32, 1024, 8, 20000, False, True, True, True, True, True, 0),
    # shared x, ragged B, no grad_x: g 2.16 GB + x 0.14 GB, counted as 2 x 2.16 GB = 4.33 GB >= 4 GiB: long stream order
    # without the stores; 16 x 128 blocks
    ("shared_no_gx", torch.float32, 1024, 16, 33001, True, True, False, True, False, False, 0),
    # float64 at D = 2048 (4 chunks per thread): 3 x 0.20 GB = 0.59 GB, the NT path
    ("f64_d2048", torch.float64, 2048, 4, 3001, False, True, True, False, True, True, 0),
    # 3 x 1.47 GB = 4.42 GB >= 4 GiB: long stream, 256 slabs x 8 = 2048 blocks; a few rows of x and g hold inf / NaN
    ("long_nonfinite", torch.float32, 1024, 8, 45000, False, True, True, False, True, True, 6),
]


def _stream_bytes(case):
    _, dtype, D, S, B, _, _, _, _, _, need_gx, _ = case
    return S * B * D * dtype.itemsize * (3 if need_gx else 2)      # what the dispatch compares with its thresholds


def _guarded(shape, dtype):
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + 2 * PAD,), SENT[dtype], device=DEV, dtype=dtype)
    return buf, buf[PAD:PAD + n].view(shape)


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _intact(buf, view):
    """No element of the margins around ``view`` changed (compared as bits)."""
    off = view.data_ptr() - buf.data_ptr()
    n = off // buf.element_size()
    sent = _bits(torch.full((1,), SENT[buf.dtype], device=DEV, dtype=buf.dtype))
    return bool((_bits(buf[:n]) == sent).all()) and bool((_bits(buf[n + view.numel():]) == sent).all())


def _operands(case, seed=1):
    name, dtype, D, S, B, shared, mean_plus, has_bias, _, _, _, poison = case
    g = torch.Generator(device=DEV).manual_seed(seed)
    kw = dict(device=DEV, dtype=dtype, generator=g)
    s1, s2 = torch.randn(D, **kw), torch.randn(D, **kw)
    u = torch.randn(S + (1 if mean_plus else 0), D, **kw) * (0.3 / D)        # the scale the reparameterisation gives
    bias = torch.randn(D, **kw) * 0.3 if has_bias else None
    x = torch.randn((B, D) if shared else (S, B, D), **kw)
    gout = torch.randn(S, B, D, **kw)
    if poison:
        gen = torch.Generator().manual_seed(seed)
        for i in range(poison):
            k, b, j = (int(torch.randint(0, n, (1,), generator=gen)) for n in (S, B, D))
            val = (float("inf"), float("-inf"), float("nan"))[i % 3]
            if i % 2:
                gout[k, b, j] = val
            else:
                x[k, b, j] = val
    return x, gout, s1, s2, u, bias


def _launch(case, ops, tune):
    """whvi_diag_apply_bwd through the C ABI into sentinel-filled, sentinel-guarded buffers: (grad_x or None, out, part),
    the selected kernel's name, and whether every margin is intact."""
    name, dtype, D, S, B, shared, mean_plus, _, relu_in, relu_out, need_gx, _ = case
    x, gout, s1, s2, u, bias = ops
    L = _hip.lib()
    log2d = D.bit_length() - 1
    n_slabs = int(L.whvi_diag_apply_bwd_slabs(0 if dtype == torch.float32 else 1, S, B, log2d))
    gxb, gx = _guarded((S, B, D), dtype) if need_gx else (None, None)
    outb, out = _guarded((4, u.shape[0], D), dtype)
    partb, part = _guarded((S, n_slabs, 2, D), dtype)
    flags = ((_hip.DIAG_X_SHARED if shared else 0) | (_hip.DIAG_MEAN_PLUS if mean_plus else 0) |
             (_hip.DIAG_RELU_IN if relu_in else 0) | (_hip.DIAG_RELU_OUT if relu_out else 0) | tune)
    fn = getattr(L, "whvi_diag_apply_bwd_" + ("f32" if dtype == torch.float32 else "f64"))
    rc = fn(None if gx is None else gx.data_ptr(), out.data_ptr(), part.data_ptr(), gout.data_ptr(), x.data_ptr(), s1.data_ptr(),
            s2.data_ptr(), u.data_ptr(), None if bias is None else bias.data_ptr(), S, B, log2d, n_slabs, flags, None)
    kernel = _hip.last_kernel()
    torch.cuda.synchronize()
    assert rc == 0, _hip.last_error()
    intact = all(_intact(b, v) for b, v in ((gxb, gx), (outb, out), (partb, part)) if b is not None)
    return gx, out, part, kernel, n_slabs, intact


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    diff = _bits(a) != _bits(b)
    assert not bool(diff.any()), (what, int(diff.sum()), diff.nonzero()[:8].tolist())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_diag_apply_bwd_paths_agree_bit_for_bit_and_stay_inside_their_buffers(case, hip_lib):
    name, dtype, D, S, B, shared, mean_plus, _, _, _, need_gx, _ = case
    ops = _operands(case)
    nbytes = _stream_bytes(case)
    long_stream = nbytes >= LONG_STREAM_BYTES
    # the sizes are chosen on the side of each threshold the case name says: a retuned threshold fails here instead of
    # silently dropping the path from the suite
    assert long_stream == (name in ("config4_share", "long_odd_grid", "shared_no_gx", "long_nonfinite")), (name, nbytes / GiB)
    assert nbytes > NT_MIN_BYTES
    tname = "float" if dtype == torch.float32 else "double"
    head = f"whvi::diag_apply_bwd_kernel<{tname}, {D.bit_length() - 1}, "
    tail = f", {'true' if shared else 'false'}, {'true' if need_gx else 'false'}>"
    ref = None
    for path, tune in PATHS.items():
        gx, out, part, kernel, n_slabs, intact = _launch(case, ops, tune)
        nt = path != "cached"                                             # every case streams more than NT_MIN_BYTES
        assert kernel == head + ("true" if nt else "false") + tail, (path, kernel)
        if path == "default" and long_stream:
            # XCD-contiguous block order only when the grid is a multiple of 8 (a bijection), as the case comments say
            assert ((n_slabs * S) % 8 == 0) == (name != "long_odd_grid"), (name, n_slabs, S)
        assert intact, (path, "a byte outside grad_x / out / part changed")
        # every output element written (a missing store shows as the sentinel)
        if gx is not None:
            assert not bool((_bits(gx) == _bits(torch.tensor(SENT[dtype], device=DEV, dtype=dtype))).any()), (path, "grad_x")
        assert not bool((part == SENT[dtype]).any()), (path, "part")
        assert not bool((out[:, 1 if mean_plus else 0:] == SENT[dtype]).any()), (path, "out")
        # (mean_plus: row 0 of every slot is the caller's, left untouched)
        assert not mean_plus or bool((out[:, 0] == SENT[dtype]).all())
        if ref is None:
            ref = (gx, out, part)
            continue
        if gx is not None:
            _same_bits(gx, ref[0], (path, "grad_x"))
        _same_bits(out, ref[1], (path, "out"))
        _same_bits(part, ref[2], (path, "part"))
        del gx, out, part
    # (b) against a plain reference, on the default path's results
    _check_vs_reference(case, ops, ref[0], ref[1])


def _check_vs_reference(case, ops, gx, out):
    name, dtype, D, S, B, shared, mean_plus, _, relu_in, relu_out, need_gx, _ = case
    x, gout, s1, s2, u, bias = ops
    # w_k by the kernel's own chain (the reference ops of DiagApplyFunction: u * s2, D * ., s1 * ., mean + sample), exactly:
    # a product with 1 changes no bit
    w = DiagApplyFunction._reference_ops(torch.ones(1, D, device=DEV, dtype=dtype), s1, s2, u, None, mean_plus).view(S, D)
    Dd = float(D)
    mp = 1 if mean_plus else 0
    a, c = s1.double(), s2.double()
    u0 = u[0].double() if mean_plus else torch.zeros_like(a)
    for k in range(S):
        xk = x if shared else x[k]
        xv = torch.relu(xk) if relu_in else xk                       # (NaN stays NaN, as relu_ in the kernel)
        g = gout[k]
        if relu_out:
            # the forward's pre-activation recomputed with its roundings; the gradient passes unless it is <= 0 (NaN passes)
            z = xv * w[k]
            if bias is not None:
                z = z + bias
            g = torch.where(z <= 0, torch.zeros((), device=DEV, dtype=dtype), g)
            del z
        if need_gx:
            want = g * w[k]
            if relu_in:
                want = torch.where(xv <= 0, torch.zeros((), device=DEV, dtype=dtype), want)
            na, nb = torch.isnan(gx[k]), torch.isnan(want)
            assert torch.equal(na, nb), (k, "grad_x NaN pattern", int((na != nb).sum()))
            _same_bits(torch.where(na, torch.zeros((), device=DEV, dtype=dtype), gx[k]),
                       torch.where(nb, torch.zeros((), device=DEV, dtype=dtype), want), (k, "grad_x vs g * w_k"))
            del want, na, nb
        gd, xd = g.double(), xv.double()
        prod = gd * xd
        sw, aw = prod.sum(0), prod.abs().sum(0)                       # sum_b g x and its A64
        sb, ab = gd.sum(0), gd.abs().sum(0)
        del prod, gd, xd
        uk = u[mp + k].double()
        refs = [(sw * (a * Dd * c), aw * (a * Dd * c).abs()),
                (sw * (Dd * (u0 * c) + Dd * (uk * c)), aw * ((Dd * (u0 * c)).abs() + (Dd * (uk * c)).abs())),
                (sw * (a * Dd * (u0 + uk)), aw * (a.abs() * Dd * (u0.abs() + uk.abs()))),
                (sb, ab)]
        for slot, (want, A) in enumerate(refs):
            got = out[slot, mp + k].double()
            fin = torch.isfinite(want)
            assert torch.equal(torch.isfinite(got), fin), (k, slot, "non-finite pattern")
            assert torch.equal(torch.isnan(got[~fin]), torch.isnan(want[~fin])), (k, slot, "NaN pattern")
            err = (got[fin] - want[fin]).abs()
            bad = err > 1e-5 * A[fin]
            assert not bool(bad.any()), (k, slot, int(bad.sum()), float((err / A[fin].clamp_min(1e-300)).max()))


# ---- (c): the torch-op backwards around it, at config 4's lengths
def _bound(got, ref, A, what):
    err = (got.double() - ref).abs()
    bad = err > 1e-5 * A
    assert not bool(bad.any()), (what, int(bad.sum()), float((err / A.clamp_min(1e-300)).max()))


@pytest.fixture(scope="module")
def config4_chain(hip_lib):
    """The operands test_config4_share_full_size draws (45 730 rows, 16 samples, K = 4 -> 1024 -> 1024 -> 1, biases and both
    ReLUs), pushed through the batched route's forward: x and W of the stacked layer, its output, the square layer's output,
    and the gradients each layer's backward receives."""
    S, B = 16, 45730
    ops, _, g = _net_operands(4, 1024, 1, S, B, (True, True, True), seed=11)
    with torch.no_grad():
        h0 = SmallKApplyFunction.apply(ops["x"], ops["w_in"], ops["b_in"], True)
    h0 = h0.requires_grad_(True)
    h1 = DiagApplyFunction.apply(h0, ops["s1"][0], ops["s2"][0], ops["u"][0], ops["b_mid"][0], S, True, False, True)
    h1d = h1.detach()
    gh1 = g.unsqueeze(-1) * ops["w_out"].unsqueeze(1)          # RowDotFunction.backward's grad_x (checked below)
    gh0, = torch.autograd.grad(h1, h0, gh1)
    del h1, gh1
    yield dict(ops=ops, g=g, h0=h0.detach(), h1=h1d, gh0=gh0, S=S, B=B)


def test_row_dot_backward_at_config4_length(config4_chain):
    c = config4_chain
    h1, w, g, S = c["h1"], c["ops"]["w_out"], c["g"], c["S"]
    xl, wl = h1.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = RowDotFunction.apply(xl, wl, False)
    gx, gw = torch.autograd.grad(y, (xl, wl), g.unsqueeze(-1))
    del xl, y
    for s in range(S):
        hs, gs = h1[s].double(), g[s].double().unsqueeze(1)
        _bound(gw[s], (hs * gs).sum(0), (hs.abs() * gs.abs()).sum(0), ("grad_w", s))        # a sum over 45 730 rows
        _bound(gx[s], gs * w[s].double(), (gs * w[s].double()).abs(), ("grad_x", s))
        del hs, gs


def test_small_k_apply_backward_at_config4_length(config4_chain):
    c = config4_chain
    ops, h0, gh0, S = c["ops"], c["h0"], c["gh0"], c["S"]
    x, W, b = ops["x"], ops["w_in"], ops["b_in"]
    leaves = [t.clone().requires_grad_(True) for t in (x, W, b)]
    out = SmallKApplyFunction.apply(*leaves, True)
    assert torch.equal(out.detach(), h0)
    gx, gW, gb = torch.autograd.grad(out, leaves, gh0)
    del out
    xd = x.double()
    ref_x, A_x = torch.zeros_like(xd), torch.zeros_like(xd)
    ref_b, A_b = torch.zeros(b.numel(), dtype=torch.float64, device=DEV), torch.zeros(b.numel(), dtype=torch.float64, device=DEV)
    for s in range(S):
        gs = torch.where(h0[s] > 0, gh0[s], torch.zeros((), device=DEV)).double()           # the ReLU behind the layer
        Ws = W[s].double()
        ref_x += gs @ Ws                                                                   # a sum over 16 x 1024 terms
        A_x += gs.abs() @ Ws.abs()
        _bound(gW[s], gs.t() @ xd, gs.abs().t() @ xd.abs(), ("grad_W", s))                 # a sum over 45 730 rows
        ref_b += gs.sum(0)                                                                 # 16 x 45 730 terms
        A_b += gs.abs().sum(0)
        del gs
    _bound(gx, ref_x, A_x, "grad_x")
    _bound(gb.reshape(-1), ref_b, A_b, "grad_bias")
