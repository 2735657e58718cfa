"""Every shipped instantiation of the regression network's kernels against a plain high-precision reference, one case each
from tools/kernel_table.py's case list (tests/test_kernel_table_host.py checks that the list reaches exactly the shipped set).

Each case runs through the C ABI into output buffers with sentinel margins whose contents are prefilled with a NaN payload no
kernel produces, and checks:
  * whvi_last_kernel == the dispatch mirror's symbol (which checks the mirror too), and for the streaming small_k_apply /
    row_dot launches the side of the XCD-reorder condition (grid % 8 == 0) the case asks for, at this device's CU count;
  * every output element written, every margin intact;
  * the values, per element:
      small_k_apply : err <= 2e-6 A64 on random weights (A64: the float64 sum of the absolute values of the element's terms);
                      on the as-written block-diagonal weights bit for bit the single rounded product, + 0 (no -0), the
                      bias and the ReLU, with a row holding inf / NaN poisoned through the exact zeros;
      row_dot       : err <= 1e-5 A64, relu_in on and off, non-finite rows where the float64 sum has them;
      diag_apply    : bit for bit the one-rounding x . w_k + 0 (+ bias), the matrix route's contract (poisoned rows included);
      diag_apply_bwd: grad_x bit for bit, the four out slots inside the float64 bound (tests/test_batched_bwd_gpu.py);
      mlp_apply     : bit-identical to the batched route's three launches;
      mlp_apply_bwd : the same bits as the plain call, and every gradient inside the float64 bound of
                      tests/test_mlp_train_gpu.py::test_gradients_inside_the_float64_bound.
References are formed on the device one sample at a time, so config 4's 3 GB outputs need no host copy."""
import os
import sys

import pytest
import torch

from whvi_amd import _hip
from whvi_amd.weights import DiagApplyFunction

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import kernel_table as kt  # noqa: E402
from test_batched_bwd_gpu import PAD, SENT, _bits, _check_vs_reference  # noqa: E402
from test_batched_bwd_gpu import _operands as _diag_operands  # noqa: E402
from test_mlp_apply_gpu import _same, _three_launches  # noqa: E402
from test_mlp_train_gpu import _check_bound_ops  # noqa: E402
from test_mlp_train_gpu import _operands as _net_operands  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
DTYPE = {"float": torch.float32, "double": torch.float64}
FILL = {torch.float32: 0x7FC5A5A5, torch.float64: 0x7FF8A5A5A5A5A5A5}      # quiet NaNs with a payload arithmetic never makes


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _cases(fam):
    return pytest.mark.parametrize("case", [c for c in kt.CASES if c["family"] == fam], ids=lambda c: c["id"])


def _guarded(shape, dtype):
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + 2 * PAD,), SENT[dtype], device=DEV, dtype=dtype)
    _bits(buf[PAD:PAD + n]).fill_(FILL[dtype])
    return buf, buf[PAD:PAD + n].view(shape)


def _intact(buf, view):
    n = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    sent = _bits(torch.full((1,), SENT[buf.dtype], device=DEV, dtype=buf.dtype))
    return bool((_bits(buf[:n]) == sent).all()) and bool((_bits(buf[n + view.numel():]) == sent).all())


def _unwritten(view):
    return int((_bits(view) == FILL[view.dtype]).sum())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _launched(case, rc):
    """After a launch: it succeeded, and the kernel it ran is the mirror's (at the grid side the case asks for)."""
    kernel = _hip.last_kernel()
    torch.cuda.synchronize()
    assert rc == 0, _hip.last_error()
    want = kt.launch(case, _cus())
    assert kernel == want.symbol, (kernel, want.symbol)
    if case.get("xcd") is not None:
        assert want.xcd == case["xcd"], (case["id"], want.grid)


def _bits_equal(got, want, what):
    """NaN exactly where the reference has NaN; every other element the same bits (so +0 and -0 differ)."""
    ng, nw = torch.isnan(got), torch.isnan(want)
    assert torch.equal(ng, nw), (what, "NaN pattern", int((ng != nw).sum()))
    diff = _bits(got[~ng]) != _bits(want[~nw])
    assert not bool(diff.any()), (what, int(diff.sum()), "of", int(diff.numel()))


def _per_element(got, ref, A, tol, what):
    """Non-finite where the float64 value is (same value), elsewhere |got - ref| <= tol A64."""
    got = got.double()
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin), (what, "non-finite pattern", int((torch.isfinite(got) != fin).sum()))
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), (what, "NaN pattern")
    inf = torch.isinf(ref)
    assert torch.equal(got[inf], ref[inf]), (what, "inf signs")
    err = (got[fin] - ref[fin]).abs()
    bad = err > tol * A[fin]
    assert not bool(bad.any()), (what, int(bad.sum()), float((err / A[fin].clamp_min(1e-300)).max()))


def test_xcd_sides_on_this_device(hip_lib):
    """At this device's CU count the streaming cases of both layer products reach both sides of the reorder condition."""
    cus = _cus()
    for fam in ("small_k_apply", "row_dot"):
        sides = {kt.launch(kt.sized(c, cus), cus).xcd for c in kt.CASES if c["family"] == fam and c.get("xcd") is not None}
        assert sides == {True, False}, fam


# ---- small_k_apply: out[s, b, n] = sum_c x[b, c] W[s, n, c] (+ bias[n]) (relu)
def _small_k_launch(case, x, w, bias):
    S, B, N, K = case["S"], case["B"], case["N"], case["K"]
    buf, out = _guarded((S, B, N), F32)
    rc = _hip.lib().whvi_small_k_apply_f32(out.data_ptr(), x.data_ptr(), w.data_ptr(), _ptr(bias), S, B, N, K.bit_length() - 1,
                                           _hip.APPLY_RELU_OUT if case["relu_out"] else 0, None)
    _launched(case, rc)
    assert _intact(buf, out), "a byte outside out changed"
    assert _unwritten(out) == 0, "elements never written"
    return out


@_cases("small_k_apply")
def test_small_k_apply(case, hip_lib):
    case = kt.sized(case, _cus())
    S, B, N, K = case["S"], case["B"], case["N"], case["K"]
    g = torch.Generator(device=DEV).manual_seed(B + N + K)
    x = torch.randn(B, K, device=DEV, generator=g)
    w = torch.randn(S, N, K, device=DEV, generator=g)
    bias = torch.randn(N, device=DEV, generator=g) if case["bias"] else None
    # random weights: every element inside 2e-6 of its A64
    out = _small_k_launch(case, x, w, bias)
    xd = x.double()
    for s in range(S):
        ref, A = xd @ w[s].double().t(), xd.abs() @ w[s].double().abs().t()
        if bias is not None:
            ref, A = ref + bias.double(), A + bias.double().abs()
        if case["relu_out"]:
            ref = torch.relu(ref)
        _per_element(out[s], ref, A, 2e-6, ("random", s))
        del ref, A
    del out
    # the as-written block-diagonal weights (one non-zero per row of W): the single rounded product + 0, bit for bit; a
    # non-finite input poisons the rest of its row through the exact zeros (inf * 0, NaN * 0)
    cols = torch.arange(N, device=DEV) % K
    wd = torch.zeros_like(w)
    wd[:, torch.arange(N, device=DEV), cols] = w[:, torch.arange(N, device=DEV), cols]
    del w
    x[1, 0], x[2, K - 1], x[3, 1] = float("inf"), float("nan"), float("-inf")
    x[4], x[0, 0], x[5, 2] = 0.0, -0.0, -0.0                       # zero products of both signs: the accumulator's +0
    out = _small_k_launch(case, x, wd, bias)
    nonfin = ~torch.isfinite(x)
    poisoned = (nonfin.sum(1, keepdim=True) - nonfin[:, cols].int()) > 0          # (B, N): another column is non-finite
    for s in range(S):
        want = x[:, cols] * wd[s, torch.arange(N, device=DEV), cols] + 0.0
        if bias is not None:
            want = want + bias
        want = torch.where(poisoned, torch.full((), float("nan"), device=DEV), want)
        if case["relu_out"]:
            want = torch.relu(want)
        _bits_equal(out[s], want, ("block-diagonal", s))
        del want
    assert bool(torch.isnan(out[:, 1, 1::K]).all()) and not bool(torch.isnan(out[:, 1, 0::K]).any())


# ---- row_dot: y[s, b] = sum_i relu?(x[s, b, i]) w[s, i] (+ bias)
@_cases("row_dot")
def test_row_dot(case, hip_lib):
    case = kt.sized(case, _cus())
    S, B, L = case["S"], case["B"], case["log2d"]
    D = 1 << L
    g = torch.Generator(device=DEV).manual_seed(B + L)
    x = torch.randn(S, B, D, device=DEV, generator=g)
    w = torch.randn(S, D, device=DEV, generator=g)
    bias = torch.randn(1, device=DEV, generator=g) if case["bias"] else None
    if case["poison"]:
        x[0, 1, D // 2], x[S - 1, B - 1, 0], x[0, 2, D - 1] = float("nan"), float("inf"), float("-inf")
    buf, y = _guarded((S, B), F32)
    rc = _hip.lib().whvi_row_dot_f32(y.data_ptr(), x.data_ptr(), w.data_ptr(), _ptr(bias), S, B, L,
                                     _hip.APPLY_RELU_IN if case["relu_in"] else 0, None)
    _launched(case, rc)
    assert _intact(buf, y), "a byte outside y changed"
    assert _unwritten(y) == 0, "rows never written"
    for s in range(S):
        xs = torch.relu(x[s]).double() if case["relu_in"] else x[s].double()
        prod = xs * w[s].double()
        ref, A = prod.sum(1), prod.abs().sum(1)
        del prod, xs
        if bias is not None:
            ref, A = ref + bias.double(), A + bias.double().abs()
        _per_element(y[s], ref, A, 1e-5, s)
    if case["poison"]:
        assert bool(torch.isnan(y[0, 1])) and bool(torch.isinf(y[S - 1, B - 1]))


# ---- diag_apply: out[k, b, :] = relu?(relu?(x[(k,) b, :]) * w_k + 0 (+ bias))
def _diag_tuple(case, need_gx):
    return (case["id"], DTYPE[case["dtype"]], 1 << case["log2d"], case["S"], case["B"], case["shared"], case["mean_plus"],
            case["bias"], case["relu_in"], case["relu_out"], need_gx, case["poison"])


def _flags(case):
    return ((_hip.DIAG_X_SHARED if case["shared"] else 0) | (_hip.DIAG_MEAN_PLUS if case["mean_plus"] else 0) |
            (_hip.DIAG_RELU_IN if case["relu_in"] else 0) | (_hip.DIAG_RELU_OUT if case["relu_out"] else 0) | case["tune"])


@_cases("diag_apply")
def test_diag_apply(case, hip_lib):
    dtype, S, B, L = DTYPE[case["dtype"]], case["S"], case["B"], case["log2d"]
    D = 1 << L
    x, _, s1, s2, u, bias = _diag_operands(_diag_tuple(case, False), seed=B + L)
    rows = x.view(-1, D)
    rows[1, : D // 2], rows[2, : D // 2] = -0.0, 0.0                 # zero products of both signs
    buf, out = _guarded((S, B, D), dtype)
    fn = getattr(_hip.lib(), "whvi_diag_apply_" + ("f32" if dtype == F32 else "f64"))
    rc = fn(out.data_ptr(), x.data_ptr(), s1.data_ptr(), s2.data_ptr(), u.data_ptr(), _ptr(bias), S, B, L, _flags(case), None)
    _launched(case, rc)
    assert _intact(buf, out), "a byte outside out changed"
    assert _unwritten(out) == 0, "elements never written"
    # w_k by the kernel's own chain (DiagApplyFunction's reference ops; a product with 1 changes no bit)
    w = DiagApplyFunction._reference_ops(torch.ones(1, D, device=DEV, dtype=dtype), s1, s2, u, None, case["mean_plus"]).view(S, D)
    nan = torch.full((), float("nan"), device=DEV, dtype=dtype)
    for k in range(S):
        xv = x if case["shared"] else x[k]
        if case["relu_in"]:
            xv = torch.relu(xv)
        want = xv * w[k] + 0.0
        if bias is not None:
            want = want + bias
        nonfin = ~torch.isfinite(xv)
        want = torch.where((nonfin.sum(-1, keepdim=True) - nonfin.int()) > 0, nan, want)      # the row's other columns
        if case["relu_out"]:
            want = torch.relu(want)
        _bits_equal(out[k], want, k)


# ---- diag_apply_bwd: grad_x and the four batch-sum slots
@_cases("diag_apply_bwd")
def test_diag_apply_bwd(case, hip_lib):
    dtype, S, B, L = DTYPE[case["dtype"]], case["S"], case["B"], case["log2d"]
    D = 1 << L
    gx_wanted = case["need_grad_x"]
    tup = _diag_tuple(case, gx_wanted)
    ops = _diag_operands(tup, seed=B + L + 1)
    x, gout, s1, s2, u, bias = ops
    L_ = _hip.lib()
    n_slabs = int(L_.whvi_diag_apply_bwd_slabs(0 if dtype == F32 else 1, S, B, L))
    assert n_slabs * S == kt.launch(case, _cus()).grid
    gxb, gx = _guarded((S, B, D), dtype) if gx_wanted else (None, None)
    outb, out = _guarded((4, u.shape[0], D), dtype)
    partb, part = _guarded((S, n_slabs, 2, D), dtype)
    fn = getattr(L_, "whvi_diag_apply_bwd_" + ("f32" if dtype == F32 else "f64"))
    rc = fn(_ptr(gx), out.data_ptr(), part.data_ptr(), gout.data_ptr(), x.data_ptr(), s1.data_ptr(), s2.data_ptr(),
            u.data_ptr(), _ptr(bias), S, B, L, n_slabs, _flags(case), None)
    _launched(case, rc)
    for b, v in ((gxb, gx), (outb, out), (partb, part)):
        if b is not None:
            assert _intact(b, v), "a byte outside grad_x / out / part changed"
    mp = 1 if case["mean_plus"] else 0
    assert _unwritten(part) == 0 and _unwritten(out[:, mp:]) == 0 and (gx is None or _unwritten(gx) == 0), "never written"
    assert _unwritten(out[:, :mp]) == out[:, :mp].numel(), "mean_plus: row 0 of every slot is the caller's"
    _check_vs_reference(tup, ops, gx, out)


# ---- mlp_apply: the one-launch predictive pass == the batched route's three launches, bit for bit
def _biases(case):
    return (case["b_in"],) + tuple(bool((case["mid_bias"] >> m) & 1) for m in range(case["n_mid"])) + (case["b_out"],)


@_cases("mlp_apply")
def test_mlp_apply(case, hip_lib):
    kin, n_mid, L, S, B = case["kin"], case["n_mid"], case["log2d"], case["S"], case["B"]
    ops, mid_bias, _ = _net_operands(kin, 1 << L, n_mid, S, B, _biases(case), seed=L * 10 + kin)
    assert mid_bias == case["mid_bias"]
    if case["poison"]:
        ops["x"][3, 0], ops["x"][5, kin - 1], ops["x"][7, 0] = float("inf"), float("nan"), float("-inf")
    buf, y = _guarded((S, B), F32)
    p = lambda k: _ptr(ops[k])  # noqa: E731
    rc = _hip.lib().whvi_mlp_apply_f32(y.data_ptr(), p("x"), kin, p("w_in"), p("b_in"), n_mid, p("s1"), p("s2"), p("u"),
                                       p("b_mid"), mid_bias, p("w_out"), p("b_out"), S, B, L, case["relu"], None)
    _launched(case, rc)
    assert _intact(buf, y), "a byte outside y changed"
    assert _unwritten(y) == 0, "rows never written"
    want = _three_launches(ops["x"], ops["w_in"], ops["b_in"], ops["s1"], ops["s2"], ops["u"], ops["b_mid"], mid_bias,
                           ops["w_out"], ops["b_out"], case["relu"], S)
    _same(y, want.contiguous())


# ---- mlp_apply_bwd: every gradient inside the float64 bound
@_cases("mlp_apply_bwd")
def test_mlp_apply_bwd(case, hip_lib):
    kin, n_mid, L, S, B, relu = case["kin"], case["n_mid"], case["log2d"], case["S"], case["B"], case["relu"]
    D = 1 << L
    need_x = case["need_grad_x"]
    ops, mid_bias, g = _net_operands(kin, D, n_mid, S, B, case["biases"], seed=L * 10 + kin + n_mid)
    lib = _hip.lib()
    need = int(lib.whvi_mlp_apply_bwd_workspace(S, B, kin, n_mid, L))
    shapes = {"gwi": (S, D) if kin == 1 else (S, D, kin), "gwm": (n_mid, S, D), "gwo": (S, D), "gb": ((1 + n_mid) * D + 1,),
              "work": (max(need, 1),)}
    if need_x:
        shapes["gx"] = (S, B, kin)
    bufs = {k: _guarded(shape, F32) for k, shape in shapes.items()}
    o = lambda k: bufs[k][1].data_ptr() if k in bufs else None  # noqa: E731
    p = lambda k: _ptr(ops[k])  # noqa: E731
    rc = lib.whvi_mlp_apply_bwd_f32(o("gwi"), o("gwm"), o("gwo"), o("gb"), o("gx"), o("work"), need, g.data_ptr(), p("x"), kin,
                                    p("w_in"), p("b_in"), n_mid, p("s1"), p("s2"), p("u"), p("b_mid"), mid_bias, p("w_out"), S, B, L,
                                    relu, None)
    _launched(case, rc)
    for k, (buf, view) in bufs.items():
        assert _intact(buf, view), k
        if k != "work":
            assert _unwritten(view) == 0, k
    want = _hip.mlp_apply_bwd(g, ops["x"], ops["w_in"], ops["b_in"], ops["s1"], ops["s2"], ops["u"], ops["b_mid"], ops["w_out"],
                              mid_bias=mid_bias, relu=relu, need_grad_x=need_x)
    for k, wt in zip(("gwi", "gwm", "gwo", "gb", "gx"), want):
        if wt is not None:
            _same(bufs[k][1], wt)
    _check_bound_ops(ops, g, mid_bias, relu, S, need_x)
