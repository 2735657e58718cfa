"""Every reachable instantiation of the weight-construction kernels (wbar_fwd_kernel, wbar_bwd_kernel) against exact references,
one launch per case of tools/wbar_table.py (tests/test_wbar_table_host.py checks that the list reaches exactly the shipped set).

The as-written matrix is exactly diagonal: W[j,k] = diag(s1 . (D . (u . s2))), one rounding per product, D . x
exact.  So the forward has a closed form in its own type for the WHOLE output, and the backward a float64 one.  Each case runs
through the C ABI into outputs with sentinel margins whose interior is prefilled with a NaN payload no kernel produces:

  common   return code 0; whvi_last_kernel == the mirror's symbol; margins intact; exactly the contract's elements written (forward:
           all of (J, S, R, D); backward: the first R entries of the sample rows of the three outputs -- entries i >= R and, under
           MEAN, row 0 of each j keep the fill); a second call gives the same bits.
  (a)      forward, whole output == the closed form in the kernel's type (+ base; the mean form: mean term + sample term), element
           for element after + 0.0; and four sampled rows (first, last, either side of a matrix boundary) bit for bit against
           oracle.pipeline on the host, so the closed form is not the only witness.
  (b)      backward on +-1 operands and a grad_w of three small integers per row: every partial sum of either network is an
           integer below 2^24, so the three outputs EQUAL the float64 closed form.
  (c)      backward on Gaussian operands, per element: |got - ref64| <= gamma_n A, n the roundings on the longest path
           (tools/wbar_table.py: roundings), A = D |s1| (sum_d |gW[i, d]|) |s2| (grad_u), ... |usum| (part_s2), |ref64| (part_s1).
  (d)      +inf, -inf and NaN planted in two rows of grad_w / entries of u, one cached and one streaming case per (entry, type,
           network): every other row keeps the bits of the clean run, the affected rows agree with the entry called on that
           one matrix alone.
  (e)      the symbols launched over the whole list are exactly ``reached()``.
References are formed on the device, a slab of matrices at a time; the only host copies are the sampled rows of (a)."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle
from whvi_amd import _hip

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import wbar_table as wt  # noqa: E402
from test_kernel_table_gpu import FILL, _bits, _guarded, _intact, _ptr, _unwritten  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPE = {"float": torch.float32, "double": torch.float64}
EPS = {"float": 2.0 ** -24, "double": 2.0 ** -53}
SLAB_BYTES = 64 << 20                         # references are formed on this much output at a time
LAUNCHED = {}                                 # case id -> the symbol whvi_last_kernel reported, for (e)
FWD = [c for c in wt.CASES if c["entry"] != "wbar_bwd"]
BWD = [c for c in wt.CASES if c["entry"] == "wbar_bwd"]
_ids = lambda c: c["id"]  # noqa: E731


def _seed(case, salt=0):
    return 7919 * [c["id"] for c in wt.CASES].index(case["id"]) + salt


def _gen(case, salt=0):
    return torch.Generator(device=DEV).manual_seed(_seed(case, salt))


def _sfx(case):
    return "f32" if case["dtype"] == "float" else "f64"


def _launched(case, rc):
    kernel = _hip.last_kernel()
    torch.cuda.synchronize()
    assert rc == 0, _hip.last_error()
    assert kernel == wt.launch(case).symbol, (kernel, wt.launch(case).symbol)
    LAUNCHED[case["id"]] = kernel


def _hash(t):
    """Two wrap-around sums over the bit patterns: equal for equal bits, and a moved or changed element changes them."""
    b = _bits(t).reshape(-1)
    return int(b.sum(dtype=torch.int64)), int((b[::3].sum(dtype=torch.int64) * 3 + b[1::7].sum(dtype=torch.int64)))


# ---- forward ---------------------------------------------------------------------------------------------------------------------
def _fwd_shape(case):
    """(u_group, u_first): the mean form reads (J, 1 + S, D) with the samples from row 1."""
    if case["entry"] == "wbar_fwd_mean":
        return case["S"] + 1, 1
    return case["first"] + case["S"] + case["spare"], case["first"]


def _fwd_operands(case, salt=0):
    dt, D, J, R = DTYPE[case["dtype"]], 1 << case["log2d"], case["J"], case["R"]
    g = _gen(case, salt)
    G, _ = _fwd_shape(case)
    s1, s2 = (torch.randn(J, D, device=DEV, dtype=dt, generator=g) for _ in range(2))
    u = torch.randn(J, G, D, device=DEV, dtype=dt, generator=g)
    base = torch.randn(J, R, D, device=DEV, dtype=dt, generator=g) if case.get("base") else None
    return s1, u, s2, base


def _fwd_call(case, out, s1, u, s2, base, J=None, S=None, G=None, first=None):
    """The C entry of the case on the given operands (J, S, u_group, u_first default to the case's)."""
    J, S = case["J"] if J is None else J, case["S"] if S is None else S
    g0, f0 = _fwd_shape(case)
    G, first = g0 if G is None else G, f0 if first is None else first
    if case["entry"] == "wbar_fwd_mean":
        assert G == S + 1 and first == 1
        fn = getattr(_hip.lib(), "whvi_wbar_fwd_mean_" + _sfx(case))
        return fn(out.data_ptr(), s1.data_ptr(), u.data_ptr(), s2.data_ptr(), J, S, case["R"], case["log2d"], None)
    fn = getattr(_hip.lib(), "whvi_wbar_fwd_" + _sfx(case))
    return fn(out.data_ptr(), s1.data_ptr(), u.data_ptr(), s2.data_ptr(), _ptr(base), J, S, case["R"], case["log2d"], G, first, None)


def _fwd_launch(case, ops):
    """Launch into a guarded buffer; the common checks.  Returns the output view."""
    D, J, S, R = 1 << case["log2d"], case["J"], case["S"], case["R"]
    buf, out = _guarded((J, S, R, D), DTYPE[case["dtype"]])
    _launched(case, _fwd_call(case, out, *ops))
    assert _intact(buf, out), "a byte outside the matrices changed"
    assert _unwritten(out) == 0, "elements never written"
    return buf, out


def _diag_term(s1j, urows, s2j, D):
    """s1 . (D . (u . s2)) in the operands' own type: one rounding per product, D . x exact -- asserted on the inputs."""
    p = urows * s2j
    t = D * p
    tiny = torch.finfo(p.dtype).tiny
    assert bool(torch.isfinite(t).all()) and bool(((p.abs() >= tiny) | (p == 0)).all()), "D u s2 overflows or is subnormal"
    return s1j * t


def _fwd_check_whole(case, out, s1, u, s2, base):
    D, J, S, R = 1 << case["log2d"], case["J"], case["S"], case["R"]
    _, first = _fwd_shape(case)
    mean = case["entry"] == "wbar_fwd_mean"
    step = max(1, SLAB_BYTES // (R * D * out.element_size()))
    for j in range(J):
        mean_term = _diag_term(s1[j, :R], u[j, 0, :R], s2[j, :R], D) if mean else None
        for k0 in range(0, S, step):
            k1 = min(S, k0 + step)
            ref = base[j].unsqueeze(0).repeat(k1 - k0, 1, 1) if base is not None else torch.zeros(k1 - k0, R, D, device=DEV, dtype=out.dtype)
            d = _diag_term(s1[j, :R], u[j, first + k0:first + k1, :R], s2[j, :R], D)
            if mean:
                d = mean_term + d
            ref.diagonal(dim1=1, dim2=2).add_(d)
            got = out[j, k0:k1]
            # == on values: the sign of an exact zero is exempt (x + 0.0 on both sides), a NaN on either side fails
            assert torch.equal(got, ref), (case["id"], j, k0, int((got != ref).sum()), "elements differ from the closed form")
            del ref, d


def _oracle_row(case, s1, u, s2, base, j, k, i):
    """Row i of matrix (j, k) by the CPU oracle's two-transform pipeline on the one-hot row (+ the mean matrix's / mean term's)."""
    D = 1 << case["log2d"]
    npdt = np.float32 if case["dtype"] == "float" else np.float64
    _, first = _fwd_shape(case)
    x = np.zeros((1, D), dtype=npdt)
    x[0, i] = 1
    one = lambda t: np.array([t.item()], dtype=npdt)  # noqa: E731
    pipe = lambda urow: oracle.pipeline(x, one(s1[j, i]), one(u[j, urow, i]), one(s2[j, i]), n_samples=1, sample_stride=1,  # noqa: E731
                                        group_rows=1, axis="row")[0]
    row = pipe(first + k)
    if case["entry"] == "wbar_fwd_mean":
        row = pipe(0) + row
    if base is not None:
        row = base[j, i].cpu().numpy() + row
    return row


def _fwd_check_rows(case, out, s1, u, s2, base):
    S, R = case["S"], case["R"]
    rows = {0, case["J"] * S * R - 1}
    if case["J"] * S > 1:
        rows |= {R - 1, R}
    flat = out.view(-1, out.shape[-1])
    for r in sorted(rows):
        jk, i = divmod(r, R)
        j, k = divmod(jk, S)
        want = _oracle_row(case, s1, u, s2, base, j, k, i)
        got = flat[r].cpu().numpy()
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (case["id"], "row", r, "differs from the oracle")


@pytest.mark.parametrize("case", FWD, ids=_ids)
def test_forward_whole_output_exact(case, hip_lib):
    """(a)"""
    ops = _fwd_operands(case)
    buf, out = _fwd_launch(case, ops)
    _fwd_check_whole(case, out, *ops)
    _fwd_check_rows(case, out, *ops)
    h = _hash(out)
    _bits(out).fill_(FILL[out.dtype])
    _launched(case, _fwd_call(case, out, *ops))
    assert _hash(out) == h and _intact(buf, out), "a second call gives other bits"


# ---- backward --------------------------------------------------------------------------------------------------------------------
def _bwd_call(case, outs, gw, s1, u, s2, J=None, S=None):
    fn = getattr(_hip.lib(), "whvi_wbar_bwd_" + _sfx(case))
    return fn(outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), gw.data_ptr(), s1.data_ptr(), u.data_ptr(), s2.data_ptr(),
              case["J"] if J is None else J, case["S"] if S is None else S, case["R"], case["log2d"],
              wt.bwd_flags(case["mean"], case["no_lds"], case["tiles"]), None)


def _bwd_launch(case, gw, s1, u, s2):
    """Launch into three guarded buffers; the common checks.  Returns [grad_u, part_s1, part_s2] (J, U, D)."""
    D, J, S, R, m = 1 << case["log2d"], case["J"], case["S"], case["R"], int(case["mean"])
    pairs = [_guarded((J, S + m, D), DTYPE[case["dtype"]]) for _ in range(3)]
    outs = [v for _, v in pairs]
    _launched(case, _bwd_call(case, outs, gw, s1, u, s2))
    for (buf, v), name in zip(pairs, ("grad_u", "part_s1", "part_s2")):
        assert _intact(buf, v), f"a byte outside {name} changed"
        assert _unwritten(v[:, m:, :R]) == 0, f"{name}: sample entries never written"
        assert _unwritten(v[:, m:, R:]) == J * S * (D - R), f"{name}: entries i >= R written"
        assert _unwritten(v[:, :m]) == J * m * D, f"{name}: MEAN leaves row 0 to the caller"
    return pairs, outs


def _bwd_reference(case, gw, s1, u, s2):
    """float64: (grad_u, part_s1, part_s2, usum, rowabs) on the written (J, S, R) entries."""
    D, R, m = 1 << case["log2d"], case["R"], int(case["mean"])
    gii = gw.diagonal(dim1=2, dim2=3).double()                                   # (J, S, R)
    s1d, s2d, ud = s1[:, None, :R].double(), s2[:, None, :R].double(), u[:, :, :R].double()
    usum = ud[:, 1:] + ud[:, :1] if m else ud
    return D * s1d * s2d * gii, D * usum * s2d * gii, D * s1d * usum * gii, usum, gw.abs().sum(-1, dtype=torch.float64)


def _again(case, pairs, outs, ops):
    """A second call into the refilled buffers gives the same bits."""
    h = [_hash(v) for v in outs]
    for v in outs:
        _bits(v).fill_(FILL[v.dtype])
    _launched(case, _bwd_call(case, outs, *ops))
    assert [_hash(v) for v in outs] == h and all(_intact(b, v) for b, v in pairs), "a second call gives other bits"


def _signs(shape, dt, g):
    return (torch.randint(0, 2, shape, device=DEV, generator=g) * 2 - 1).to(dt)


def _integer_grad(case, g):
    """(J, S, R, D) with exactly three (D = 2: two) non-zeros in {+-1, +-2, +-3} per row, one on the diagonal in every second row."""
    dt, D, J, S, R = DTYPE[case["dtype"]], 1 << case["log2d"], case["J"], case["S"], case["R"]
    rows = J * S * R
    nz = min(3, D)
    r = torch.arange(rows, device=DEV)
    c0 = torch.where(r % 2 == 0, r % R, torch.randint(0, D, (rows,), device=DEV, generator=g))
    o1 = torch.randint(0, D - 1, (rows,), device=DEV, generator=g)
    cols = [c0, (c0 + 1 + o1) % D]
    if nz == 3:
        o2 = (o1 + 1 + torch.randint(0, D - 2, (rows,), device=DEV, generator=g)) % (D - 1)
        cols.append((c0 + 1 + o2) % D)
    vals = (torch.randint(1, 4, (rows, nz), device=DEV, generator=g) * (torch.randint(0, 2, (rows, nz), device=DEV, generator=g) * 2 - 1))
    gw = torch.zeros(rows, D, device=DEV, dtype=dt)
    gw.scatter_(1, torch.stack(cols, 1), vals.to(dt))
    return gw.view(J, S, R, D), nz


@pytest.mark.parametrize("case", BWD, ids=_ids)
def test_backward_integer_operands_exact(case, hip_lib):
    """(b)"""
    dt, D, J, S, m = DTYPE[case["dtype"]], 1 << case["log2d"], case["J"], case["S"], int(case["mean"])
    g = _gen(case, 1)
    s1, s2, u = _signs((J, D), dt, g), _signs((J, D), dt, g), _signs((J, S + m, D), dt, g)
    gw, nz = _integer_grad(case, g)
    assert bool(((gw != 0).sum(-1) == nz).all())
    pairs, outs = _bwd_launch(case, gw, s1, u, s2)
    ref_u, ref_s1, ref_s2, usum, rowabs = _bwd_reference(case, gw, s1, u, s2)
    # every partial sum of either network is an integer of at most D sum_d |gW| (1 + MEAN): below 2^24 (2^53)
    assert float(rowabs.max()) * D * (1 + m) < 1 / EPS[case["dtype"]]
    R = case["R"]
    for name, got, ref in (("grad_u", outs[0], ref_u), ("part_s1", outs[1], ref_s1), ("part_s2", outs[2], ref_s2)):
        got = got[:, m:, :R].double()
        assert torch.equal(got, ref), (case["id"], name, int((got != ref).sum()), "integers differ")
    _again(case, pairs, outs, (gw, s1, u, s2))


def _gamma(n, e):
    return n * e / (1 - n * e)


@pytest.mark.parametrize("case", BWD, ids=_ids)
def test_backward_gaussian_operands_inside_the_bound(case, hip_lib):
    """(c)  |got - ref64| <= gamma_n A per element, e = 2^-24 / 2^-53, n = tools/wbar_table.py: roundings (2 log2 D + 2 for grad_u
    and part_s2, 2 for part_s1, one more under MEAN for the rounded sum usum = u_k + u_0), A = D |s1| (sum_d |gW[i, d]|) |s2|
    for grad_u, ... |usum| for part_s2 and |ref64| for part_s1.

    Under MEAN this is the test that found the kernel adding two separately rounded products (u_k c + u_0 c, and the like for
    part_s1): where u_k and u_0 cancel the error stayed at e (|u_k| + |u_0|) ... while the result shrinks with |u_k + u_0| --
    ratios to this bound of up to 2.3e6 (part_s1, float32 D = 4, 1.54 M of 16.8 M elements over) and 1.8e6 (part_s2, float64
    D = 2) on all 78 MEAN cases, first seen on bwd_f32_L2_small_mean.  The kernel now forms u_k + u_0 once; worst ratios since, grad_u / part_s2 / part_s1:
    float32 0.52 / 0.54 / 0.99, float64 0.85 / 0.90 / 0 (float64 part_s1 is the closed form's own arithmetic)."""
    dt, D, J, S, R, m = DTYPE[case["dtype"]], 1 << case["log2d"], case["J"], case["S"], case["R"], int(case["mean"])
    g = _gen(case, 2)
    s1, s2 = (torch.randn(J, D, device=DEV, dtype=dt, generator=g) for _ in range(2))
    u = torch.randn(J, S + m, D, device=DEV, dtype=dt, generator=g)
    gw = torch.randn(J, S, R, D, device=DEV, dtype=dt, generator=g)
    _, outs = _bwd_launch(case, gw, s1, u, s2)
    ref_u, ref_s1, ref_s2, usum, rowabs = _bwd_reference(case, gw, s1, u, s2)
    rowabs = rowabs * D * s1[:, None, :R].double().abs()
    A = {"grad_u": rowabs * s2[:, None, :R].double().abs(), "part_s2": rowabs * usum.abs(), "part_s1": ref_s1.abs()}
    n = wt.roundings(wt.launch(case).policy, case["log2d"], case["mean"])
    worst = {}
    for name, got, ref in (("grad_u", outs[0], ref_u), ("part_s1", outs[1], ref_s1), ("part_s2", outs[2], ref_s2)):
        err = (got[:, m:, :R].double() - ref).abs()
        bound = _gamma(n[name], EPS[case["dtype"]]) * A[name]
        ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        worst[name] = (float(ratio.max()), int((err > bound).sum()))
        print(f"RATIO {case['id']} {name} n={n[name]} worst={worst[name][0]:.4f} over={worst[name][1]}")
    assert all(over == 0 for _, over in worst.values()), (case["id"], worst)


# ---- (d) non-finite values ---------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return bool((_bits(a.contiguous()) == _bits(b.contiguous())).all())


def _agree(got, want, what):
    """NaN and inf in the same places (same infinities), the same finite values."""
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (what, "NaN positions")
    fin = ~torch.isnan(got)
    assert torch.equal(got[fin], want[fin]), (what, "inf positions or finite values")


@pytest.mark.parametrize("case", wt.nonfinite_cases(), ids=_ids)
def test_nonfinite_values_stay_in_their_rows(case, hip_lib):
    """(d)"""
    dt, D, J, S, R = DTYPE[case["dtype"]], 1 << case["log2d"], case["J"], case["S"], case["R"]
    inf, nan = float("inf"), float("nan")
    # two rows: matrix (0, 0) row 1 and the last matrix's row R - 2 -- in different tiles, blocks and, streaming, XCDs
    spots = ((0, 0, 1), (J - 1, S - 1, R - 2))
    if case["entry"] == "wbar_bwd":
        m = int(case["mean"])
        g = _gen(case, 3)
        s1, s2 = (torch.randn(J, D, device=DEV, dtype=dt, generator=g) for _ in range(2))
        u = torch.randn(J, S + m, D, device=DEV, dtype=dt, generator=g)
        gw = torch.randn(J, S, R, D, device=DEV, dtype=dt, generator=g)
        _, clean = _bwd_launch(case, gw, s1, u, s2)
        (j0, k0, i0), (j1, k1, i1) = spots
        gw[j0, k0, i0, 3], gw[j0, k0, i0, D - 1] = inf, -inf
        gw[j1, k1, i1, i1] = nan
        _, dirty = _bwd_launch(case, gw, s1, u, s2)
        hit = torch.zeros(J, S + m, D, device=DEV, dtype=torch.bool)
        for j, k, i in spots:
            hit[j, m + k, i] = True
        for c, d in zip(clean, dirty):
            assert _same_bits(c[~hit], d[~hit]), "a row without a planted value changed"
        one = dict(case, tiles=None)                             # that one matrix alone: a cached one-matrix call
        for j, k, i in spots:
            uu = torch.stack((u[j, 0], u[j, m + k])).unsqueeze(0) if m else u[j, k].view(1, 1, D)
            alone = [torch.zeros(1, 1 + m, D, device=DEV, dtype=dt) for _ in range(3)]
            rc = _bwd_call(one, alone, gw[j, k], s1[j], uu.contiguous(), s2[j], J=1, S=1)
            assert not wt.launch(dict(one, J=1, S=1)).nt
            torch.cuda.synchronize()
            assert rc == 0, _hip.last_error()
            for d, a in zip(dirty, alone):
                _agree(d[j, m + k, i], a[0, m, i], (case["id"], j, k, i))
            assert not bool(torch.isfinite(dirty[0][j, m + k, i]))
    else:
        s1, u, s2, base = _fwd_operands(case, 3)
        _, first = _fwd_shape(case)
        _, clean = _fwd_launch(case, (s1, u, s2, base))
        (j0, k0, i0), (j1, k1, i1) = spots
        u[j0, first + k0, i0] = inf
        u[j1, first + k1, i1] = nan
        i2 = i1 - 1 if R > 2 else i1
        if i2 != i1:
            u[j1, first + k1, i2] = -inf
            spots = spots + ((j1, k1, i2),)
        _, dirty = _fwd_launch(case, (s1, u, s2, base))
        hit = torch.zeros(J, S, R, device=DEV, dtype=torch.bool)
        for j, k, i in spots:
            hit[j, k, i] = True
        assert _same_bits(clean[~hit], dirty[~hit]), "a row without a planted value changed"
        for j, k, i in spots:
            alone = torch.zeros(1, 1, R, D, device=DEV, dtype=dt)
            if case["entry"] == "wbar_fwd_mean":
                uu = torch.stack((u[j, 0], u[j, first + k])).unsqueeze(0).contiguous()
                rc = _fwd_call(case, alone, s1[j], uu, s2[j], None, J=1, S=1, G=2, first=1)
            else:
                rc = _fwd_call(case, alone, s1[j], u[j, first + k], s2[j], None if base is None else base[j], J=1, S=1, G=1, first=0)
            torch.cuda.synchronize()
            assert rc == 0, _hip.last_error()
            _agree(dirty[j, k, i], alone[0, 0, i], (case["id"], j, k, i))
            assert not bool(torch.isfinite(dirty[j, k, i]).any()), "the planted value does not fill its row"


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
def test_case_list_launches_every_reachable_instantiation(hip_lib):
    """Over the whole list whvi_last_kernel names exactly ``reached()``.  Cases (a) and (b) have not launched in this session are
    launched here on uninitialised operands: only the dispatch matters."""
    for case in wt.CASES:
        if case["id"] in LAUNCHED:
            continue
        dt, D, J, S, R = DTYPE[case["dtype"]], 1 << case["log2d"], case["J"], case["S"], case["R"]
        e = lambda *shape: torch.empty(*shape, device=DEV, dtype=dt)  # noqa: E731
        if case["entry"] == "wbar_bwd":
            m = int(case["mean"])
            rc = _bwd_call(case, [e(J, S + m, D) for _ in range(3)], e(J, S, R, D), e(J, D), torch.zeros(J, S + m, D, device=DEV, dtype=dt), e(J, D))
        else:
            G, _ = _fwd_shape(case)
            rc = _fwd_call(case, e(J, S, R, D), e(J, D), e(J, G, D), e(J, D), e(J, R, D) if case.get("base") else None)
        _launched(case, rc)
    seen = set()
    for case in wt.CASES:
        la = wt.launch(case)
        assert LAUNCHED[case["id"]] == la.symbol
        seen.add(la.shipped)
    assert seen == wt.reached() and len(seen) == 216
