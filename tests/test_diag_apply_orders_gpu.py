"""whvi_diag_apply's forward (whvi_amd/csrc/diag_apply.hpp) on each of the three orders in which diag_apply_kernel walks its
tiles, over the WHOLE output:

  plain           blk = blockIdx.x;
  XCD-contiguous  a streaming (NT) launch whose grid is a multiple of 8;
  sample-fastest  a shared input on an NT launch with S > 1 and every sample a whole number of 8-block groups -- the order
                  of a layer's first pass (forward_mc on a (batch, D) input) at stream size, the shape
                  tools/diag_apply_rate.py and the bench's fastfood-module leg time.

A block map that is not a bijection leaves tiles unwritten and writes others twice with the same values, which a comparison
of sampled rows in a torch.empty result can miss.  So every launch here goes through the C ABI into an output prefilled with
a NaN payload no arithmetic produces, between sentinel margins, and asserts
  * rc == 0 and whvi_last_kernel == the mirror's symbol (tools/kernel_table.py);
  * whvi_diag_apply_order == the mirror's order == the order the case names (kernel_table.ORDER_CASES);
  * the margins intact and no element unwritten;
  * every sample's whole output bit for bit equal to the reference tests/test_kernel_table_gpu.py::test_diag_apply uses:
    one rounding of relu?(x) * w_k + 0, then + bias, rows holding a non-finite value poisoned in their other columns, relu?
    behind; w_k from DiagApplyFunction._reference_ops in plain torch ops, formed one sample at a time on the device;
  * independently of that chain, every finite output against float64: x (wd(u0) + wd(uk)) + bias computed in float64 from
    the same operands, |got - ref| <= TOL A64 with A64 the float64 sum of the absolute values of the terms.

TOL, by counting roundings (e = half an ulp relative: 2^-24 for float32, 2^-53 for float64).  wbar_diag rounds u * s2 and
s1 * (D v) (D v is exact): wd carries 2 e.  The sum wd(u0) + wd(uk) rounds once more: w_k is within 3 e of
|wd(u0)| + |wd(uk)|.  The epilogue rounds x * w_k (4 e of |x| (|wd0| + |wdk|)) and + bias (e of the result, itself at most
(1 + 4 e) A64): 5 e A64 up to terms in e^2.  The float64 reference of a float32 launch is exact at this scale; for a
float64 launch it rounds as often as the kernel, another 5 e.  One e on top covers the second-order terms:
TOL = 6 * 2^-24 = 3.6e-7 (float32), 11 * 2^-53 (float64) -- below the 2e-6 tests/test_diag_apply_gpu.py grants this chain.
(Without the mean row, a bias or with the ReLUs there are fewer roundings; relu is 1-Lipschitz and exact.)

Every case carries exact zeros of both signs and poisoned rows (inf, -inf, NaN; one per row and several per row): on the
one-sample LDS path under the sample-fastest order, and on a block that straddles two samples under the XCD-contiguous one.

Completeness cap: zero.  No case is skipped, sampled or shortened for memory or time: every sample of every case goes whole
through the unwritten count, the bit compare and the float64 compare (the loop of _check has no early exit and takes no
subset), so the share of output elements left uncompared is 0 -- _check asserts the shapes it compared multiply out to
S * B * D.  The size-dispatched cases (512 MiB .. 4 GiB written) keep x and the references on the device, one sample at
a time."""
import os
import sys

import pytest
import torch

from whvi_amd import _hip
from whvi_amd.weights import DiagApplyFunction, WHVISquarePow2Matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import kernel_table as kt  # noqa: E402
from test_kernel_table_gpu import DTYPE, FILL, _bits_equal, _flags, _guarded, _intact, _ptr, _unwritten  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROUNDINGS = 5                                        # u * s2, s1 * ., wd0 + wdk, x * w, + bias (module docstring)
TOL = {torch.float32: (ROUNDINGS + 1) * 2.0 ** -24, torch.float64: (2 * ROUNDINGS + 1) * 2.0 ** -53}
assert all(t <= 2e-6 for t in TOL.values())


def _operands(case):
    dtype, S, B, D = DTYPE[case["dtype"]], case["S"], case["B"], 1 << case["log2d"]
    g = torch.Generator(device=DEV).manual_seed(B + case["log2d"] + S)
    kw = dict(device=DEV, dtype=dtype, generator=g)
    s1, s2 = torch.randn(D, **kw), torch.randn(D, **kw)
    u = torch.randn(S + (1 if case["mean_plus"] else 0), D, **kw) * (0.3 / D)
    bias = torch.randn(D, **kw) * 0.3 if case["bias"] else None
    x = torch.randn((B, D) if case["shared"] else (S, B, D), **kw)
    rows = x.view(-1, D)
    R = rows.shape[0]
    inf, nan = float("inf"), float("nan")
    # exact zeros of both signs (a ReLU's output; products of -0 come out as +0)
    rows[1, : max(1, D // 2)], rows[2, : max(1, D // 2)] = -0.0, 0.0
    rows[R - 2, D - 1] = -0.0
    # poisoned rows: one non-finite value per row (first, last, middle) and several per row; the first and the last row of
    # the input lie in the blocks at the sample boundaries
    rows[0, D - 1] = inf
    rows[R - 1, 0] = -inf
    rows[R // 2, D // 2] = nan
    rows[3, 0], rows[3, D - 1], rows[3, D // 2] = nan, -inf, inf
    rows[R // 2 + 1, 1], rows[R // 2 + 1, D - 2] = inf, inf
    if not case["shared"]:                            # the rows either side of the boundary between samples 0 and 1
        rows[B - 1, D // 4], rows[B, 0], rows[B, D - 1] = -inf, nan, inf
    return x, s1, s2, u, bias


def _check(case, x, s1, s2, u, bias, out):
    """The whole of ``out`` against both references, one sample at a time; returns the number of elements compared."""
    dtype, S, B, D = DTYPE[case["dtype"]], case["S"], case["B"], 1 << case["log2d"]
    mp = 1 if case["mean_plus"] else 0
    w = DiagApplyFunction._reference_ops(torch.ones(1, D, device=DEV, dtype=dtype), s1, s2, u, None, case["mean_plus"]).view(S, D)
    nan = torch.full((), float("nan"), device=DEV, dtype=dtype)
    a, c, Dd = s1.double(), s2.double(), float(D)
    wd = lambda r: a * (Dd * (u[r].double() * c))  # noqa: E731
    bd = bias.double() if bias is not None else torch.zeros(D, device=DEV, dtype=torch.float64)
    compared = n_fin = 0
    saw = set()
    for k in range(S):
        xv = x if case["shared"] else x[k]
        if case["relu_in"]:
            xv = torch.relu(xv)
        want = xv * w[k] + 0.0
        if bias is not None:
            want = want + bias
        nonfin = ~torch.isfinite(xv)
        want = torch.where((nonfin.sum(-1, keepdim=True) - nonfin.int()) > 0, nan, want)      # the row's other columns
        del nonfin
        if case["relu_out"]:
            want = torch.relu(want)
        assert out[k].shape == want.shape == (B, D)
        _bits_equal(out[k], want, (case["id"], k))
        compared += want.numel()
        saw |= {n for n, t in (("nan", torch.isnan(want).any()), ("inf", torch.isinf(want).any())) if bool(t)}
        del want
        # float64, from the same operands
        w64 = wd(mp + k) + wd(0) if mp else wd(k)
        A64 = (wd(mp + k).abs() + wd(0).abs()) if mp else wd(k).abs()
        xd = xv.double()
        ref, A = xd * w64 + bd, xd.abs() * A64 + bd.abs()
        del xd
        if case["relu_out"]:
            ref = torch.relu(ref)
        got = out[k].double()
        fin = torch.isfinite(got)
        err = (got - ref).abs()
        bad = fin & ~(err <= TOL[dtype] * A)
        assert not bool(bad.any()), (case["id"], k, int(bad.sum()), float((err[fin] / A[fin].clamp_min(1e-300)).max()))
        n_fin += int(fin.sum())
        del ref, A, got, fin, err, bad
    assert compared == S * B * D == out.numel(), "the completeness cap: whole samples, all of them"
    # (the cases' own sanity: poisoned rows are there, most of the output is finite; behind a ReLU an inf may be clamped)
    assert n_fin > 0.85 * S * B * D and "nan" in saw and (case["relu_out"] or "inf" in saw), (n_fin, saw)
    return compared


def _launch(case, x, s1, s2, u, bias, in_place=False):
    dtype, S, B, L = DTYPE[case["dtype"]], case["S"], case["B"], case["log2d"]
    D = 1 << L
    buf, out = _guarded((S, B, D), dtype)
    if in_place:
        out.copy_(x)
    src = out if in_place else x
    lib = _hip.lib()
    code = 0 if dtype == torch.float32 else 1
    c = dict(case, in_place=in_place)
    want = kt.launch(c, torch.cuda.get_device_properties(0).multi_processor_count)
    order = int(lib.whvi_diag_apply_order(code, S, B, L, _flags(case), int(in_place)))
    assert order == want.order == case["order"], (case["id"], kt.ORDER_NAMES[order], kt.ORDER_NAMES[want.order], want.grid)
    assert want.grid == case["grid"]
    fn = getattr(lib, "whvi_diag_apply_" + ("f32" if dtype == torch.float32 else "f64"))
    rc = fn(out.data_ptr(), src.data_ptr(), s1.data_ptr(), s2.data_ptr(), u.data_ptr(), _ptr(bias), S, B, L, _flags(case), None)
    kernel = _hip.last_kernel()
    torch.cuda.synchronize()
    assert rc == 0, _hip.last_error()
    assert kernel == want.symbol, (kernel, want.symbol)
    assert _intact(buf, out), "a byte outside out changed"
    if not in_place:
        n = _unwritten(out)
        if n:
            # which tiles: the first unwritten rows, as (sample, row) -- the block index follows from the tile size
            rows = (out.view(-1, D).view(torch.int64 if dtype == torch.float64 else torch.int32) == FILL[dtype]).any(1).nonzero().flatten()
            where = [(int(r) // B, int(r) % B) for r in rows[:8].tolist()]
            raise AssertionError(f"{case['id']}: {n} elements never written ({len(rows)} rows; first (sample, row): {where})")
    return buf, out


@pytest.mark.parametrize("case", kt.ORDER_CASES, ids=lambda c: c["id"])
def test_forward_on_every_block_order_over_the_whole_output(case, hip_lib):
    x, s1, s2, u, bias = _operands(case)
    D = 1 << case["log2d"]
    if case["id"] == "order_size_L10_S16_B8200":
        # the XCD-contiguous case whose blocks straddle samples: 16 rows per block, 8200 = 512 * 16 + 8 -- the poisoned first
        # and last rows of the input are computed by blocks that hold rows of two samples
        rows_per_block = 4 * 64 * 16 * (16 // x.element_size()) // D
        assert case["B"] % rows_per_block != 0
    buf, out = _launch(case, x, s1, s2, u, bias)
    assert _check(case, x, s1, s2, u, bias, out) == out.numel()
    del buf, out
    if case["in_place_too"]:
        buf, out = _launch(case, x, s1, s2, u, bias, in_place=True)
        assert _check(case, x, s1, s2, u, bias, out) == out.numel()


def test_order_cases_cover_every_order_on_this_device(hip_lib):
    """The query has the last word: on this device the cases take all three orders, and every option occurs under each."""
    lib = _hip.lib()
    seen = {}
    for c in kt.ORDER_CASES:
        o = int(lib.whvi_diag_apply_order(0 if c["dtype"] == "float" else 1, c["S"], c["B"], c["log2d"], _flags(c), 0))
        seen.setdefault(o, set()).update({("bias", c["bias"]), ("mean_plus", c["mean_plus"])} | {k for k in ("relu_in", "relu_out") if c[k]})
    assert set(seen) == {_hip.DIAG_ORDER_PLAIN, _hip.DIAG_ORDER_XCD, _hip.DIAG_ORDER_SAMPLE_FASTEST}
    for o, opts in seen.items():
        assert opts >= {("bias", True), ("bias", False), ("mean_plus", False), "relu_in", "relu_out"}, (o, opts)


def test_module_first_pass_at_stream_size_equals_the_faithful_dataflow(hip_lib):
    """WHVISquarePow2Matrix.forward_mc on a shared (8192, 1024) input, 16 samples (512 MiB written: the sample-fastest
    launch): the default route == weight construction + GEMM with the same seed, as test_module_routes checks at 40 rows."""
    torch.manual_seed(3)
    sq = WHVISquarePow2Matrix(1024, bias=True).to(DEV)
    with torch.no_grad():
        sq.g_mu.normal_()
        sq.bias.normal_()
    x = torch.randn(8192, 1024, device=DEV)
    assert _hip.diag_apply_order(torch.float32, 16, 8192, 1024, _hip.DIAG_X_SHARED | _hip.DIAG_MEAN_PLUS) == _hip.DIAG_ORDER_SAMPLE_FASTEST
    sq.faithful_dataflow = False
    torch.manual_seed(5)
    fast = sq.forward_mc(x, 16)
    assert _hip.last_kernel() == "whvi::diag_apply_kernel<float, 10, 16, true, true>", _hip.last_kernel()
    sq.faithful_dataflow = True
    torch.manual_seed(5)
    slow = sq.forward_mc(x, 16)
    assert fast.shape == (16, 8192, 1024) and torch.equal(fast, slow)
