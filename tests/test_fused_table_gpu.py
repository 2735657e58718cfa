"""Every shipped instantiation of the fused forward (fused_shs_kernel, fused_shs16_kernel) under every block map the dispatch
gives it, whole output, bit for bit: one case each from tools/fused_table.py's case list (tests/test_fused_table_host.py
checks that the list reaches exactly the shipped set and covers the (class x block map) matrix).

Each case runs through the C ABI.  Out of place the destination sits between sentinel margins and is prefilled with a NaN
payload no arithmetic produces; in place the source sits between the margins and the operands make y != x, so a tile the block
map never reaches shows in the bit compare.  Checked per case:
  * rc == 0 and whvi_last_kernel == the mirror's symbol at this device's CU count;
  * whvi_fused_shs_plan == the mirror (stage, nt, same_sample_blocks, grid) and the block map is the one the case names;
  * margins intact, no element unwritten;
  * the WHOLE output bit for bit (NaN positions, and the bits of every other element) equal to the composed chain on the
    device, a (.) fwht(b_s (.) fwht(c (.) x)) -- every multiply one torch op, every transform _hip.fwht_rows (which
    tests/test_fwht_gpu.py pins to the reference bit for bit); row-axis scales are per-row scalars, the identity source is
    built explicitly (row i of diag(c)), ONE_TRANSFORM is the half chain, SRC_SHARED the expanded input.  The chain is formed
    a slab of rows at a time and the compared slabs add up to rows x D: nothing is sampled;
  * 16-bit cases: bit for bit the float32 launch of the same arguments on the upcast input, cast once;
  * at least 64 rows bit for bit against oracle.pipeline / oracle.fwht on the CPU: the first and last row, the rows around the
    sample boundaries, the first and last row of the first, a middle and the last block under the case's block map, and
    random ones;
  * exact zeros of both signs and rows poisoned with inf, -inf and NaN in the first block, the last block and at a sample
    boundary (for the identity source, which has no rows to poison, in b): the finite rows beside them stay bit-exact.
All comparisons are bit-exact: there is no tolerance.  The last test asserts that the launches of this file reported every
shipped symbol of the two families."""
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
import fused_table as ft  # noqa: E402
from test_batched_bwd_gpu import PAD  # noqa: E402
from test_kernel_table_gpu import FILL, _bits_equal, _guarded, _intact, _unwritten  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPE = {"float": torch.float32, "double": torch.float64, "__half": torch.float16, "__hip_bfloat16": torch.bfloat16}
SUFFIX = {"float": "f32", "double": "f64", "__half": "f16", "__hip_bfloat16": "bf16"}
FILL16 = {torch.float16: 0x7EA5, torch.bfloat16: 0x7FE5}       # quiet NaNs with a payload no cast of an arithmetic result has
SENT16 = -7.25e3
SEEN = set()                                                   # every symbol whvi_last_kernel reported in this file


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _iview(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _guard(shape, dtype):
    """A buffer of ``shape`` between sentinel margins, its contents prefilled with the NaN payload."""
    if dtype in FILL:
        return _guarded(shape, dtype)
    n = shape[0] * shape[1]
    buf = torch.full((n + 2 * PAD,), SENT16, device=DEV, dtype=dtype)
    _iview(buf[PAD:PAD + n]).fill_(FILL16[dtype])
    return buf, buf[PAD:PAD + n].view(shape)


def _margins_intact(buf, view):
    if buf.dtype in FILL:
        return _intact(buf, view)
    sent = _iview(torch.full((1,), SENT16, device=DEV, dtype=buf.dtype))
    return bool((_iview(buf[:PAD]) == sent).all()) and bool((_iview(buf[PAD + view.numel():]) == sent).all())


def _never_written(view):
    if view.dtype in FILL:
        return _unwritten(view)
    return int((_iview(view) == FILL16[view.dtype]).sum())


def _same_bits(got, want, what):
    """NaN exactly where the reference has NaN; every other element the same bits."""
    if got.dtype in FILL:
        return _bits_equal(got, want, what)
    ng, nw = torch.isnan(got), torch.isnan(want)
    assert torch.equal(ng, nw), (what, "NaN pattern", int((ng != nw).sum()))
    diff = _iview(got)[~ng] != _iview(want)[~nw]
    assert not bool(diff.any()), (what, int(diff.sum()), "of", int(diff.numel()))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _boundary_row(case):
    """A row with a sample boundary in front of it."""
    stride, rows = case["sample_stride"], case["rows"]
    return stride if 1 < stride < rows - 1 else rows // 2


def _operands(case, index):
    """x (None for the identity source; sample_stride rows when shared), a, b, c (None when absent), with the special values."""
    T, L, S, stride, rows = DTYPE[case["dtype"]], case["log2d"], case["n_samples"], case["sample_stride"], case["rows"]
    D = 1 << L
    vt = torch.float32 if T in FILL16 else T                   # 16-bit activations: float32 scale vectors
    row_scales = case["axis"] == ft.AXIS_ROW or case["eye"]
    unit = case["group_rows"] if row_scales else D
    g = torch.Generator(device=DEV).manual_seed(1000 + index)
    x = None
    if not case["eye"]:
        n = stride if case["shared"] else rows
        x = torch.randn(n, D, device=DEV, dtype=torch.float32, generator=g).to(T)
        bnd = _boundary_row(case) % n
        x[0, 1 % D], x[2 % n, 0], x[n - 1, 0] = 0.0, -0.0, -0.0                                 # exact zeros of both signs
        if D > 2:                                                                                # (never a whole row of them)
            x[bnd - 1, D - 1] = 0.0
        x[1 % n, 3 % D], x[n - 2, D - 1], x[bnd, 0] = float("inf"), float("-inf"), float("nan")  # first / last block, boundary
    s = 1.0 / D ** 0.5                                         # results of order one: finite in fp16
    a = torch.randn(S if case["a_ps"] else 1, unit, device=DEV, dtype=vt, generator=g) * s if case["a"] else None
    b = torch.randn(S, unit, device=DEV, dtype=vt, generator=g) * s if case["b"] else None
    c = torch.randn(S if case["c_ps"] else 1, unit, device=DEV, dtype=vt, generator=g) if case["c"] else None
    if case["eye"] and b is not None:                          # no rows to poison: the per-row scalars of b instead
        flat = b.view(-1)
        flat[1 % flat.numel()], flat[flat.numel() - 1] = float("inf"), float("nan")
    return x, a, b, c


def _per_row(case, vec, per_sample, idx, smp):
    """The scale of rows ``idx`` (device tensor) of samples ``smp``: (n, D) column vectors or (n, 1) row scalars."""
    if case["axis"] == ft.AXIS_ROW or case["eye"]:
        g = case["group_rows"]
        return vec.view(-1)[(smp * g if per_sample else 0) + idx % g].unsqueeze(1)
    return vec[smp] if per_sample else vec[0]


def _chain(case, x, a, b, c, r0, r1):
    """Rows r0 .. r1 of the composed chain on the device: one torch op per multiply, _hip.fwht_rows per transform."""
    S, stride, D = case["n_samples"], case["sample_stride"], 1 << case["log2d"]
    idx = torch.arange(r0, r1, device=DEV)
    smp = (idx // stride) % S
    if case["eye"]:                                            # row i of diag(c): c_i at column i, +0 elsewhere
        i = idx % case["group_rows"]
        t = torch.zeros(r1 - r0, D, device=DEV, dtype=DTYPE[case["dtype"]])
        t[torch.arange(r1 - r0, device=DEV), i] = _per_row(case, c, case["c_ps"], idx, smp).view(-1) if c is not None else 1.0
    else:
        t = x[idx % stride] if case["shared"] else x[r0:r1]
        if c is not None and not case["one"]:
            t = _per_row(case, c, case["c_ps"], idx, smp) * t
    if not case["one"]:
        t = _hip.fwht_rows(t.contiguous())
    if b is not None:
        t = _per_row(case, b, True, idx, smp) * t
    t = _hip.fwht_rows(t.contiguous())
    if a is not None:
        t = _per_row(case, a, case["a_ps"], idx, smp) * t
    return t


def _launch(case, dtype_name, dst, src, a, b, c):
    fn = getattr(_hip.lib(), "whvi_fused_shs_ex_" + SUFFIX[dtype_name])
    axis = ft.AXIS_ROW if case["eye"] else case["axis"]
    rc = fn(dst.data_ptr(), _ptr(src), _ptr(a), _ptr(b), _ptr(c), case["rows"], case["log2d"], case["n_samples"], case["sample_stride"],
            case["group_rows"], axis, ft.flags_of(case), None)
    kernel = _hip.last_kernel()
    torch.cuda.synchronize()
    assert rc == 0, _hip.last_error()
    return kernel


def _oracle_rows(case, la):
    """At least 64 rows: first, last, around the sample boundaries, the ends of the first, a middle and the last block under
    the case's block map, random ones."""
    rows, stride, S = case["rows"], case["sample_stride"], case["n_samples"]
    tr = ft.tile_rows(case["dtype"], case["log2d"])
    pick = [0, rows - 1, stride - 1, stride, stride + 1, 2 * stride - 1, 2 * stride, rows - rows % stride - 1, rows - rows % stride,
            rows - stride - 1, rows - stride, _boundary_row(case) - 1, _boundary_row(case), _boundary_row(case) + 1]
    for block in (0, la.grid // 2, la.grid - 1):
        tiles = [t for t in ft.block_tiles(la, S, block) if t < la.n_tiles]
        pick += [tiles[0] * tr, tiles[0] * tr + tr - 1, tiles[-1] * tr, tiles[-1] * tr + tr - 1]
    rng = np.random.default_rng(rows)
    pick = np.concatenate([np.asarray(pick, dtype=np.int64), rng.choice(rows, min(72, rows), replace=False)])
    idx = np.unique(np.clip(pick, 0, rows - 1))
    assert len(idx) >= min(64, rows)
    return idx


def _oracle_check(case, idx, got, xs, a, b, c):
    """Rows ``idx`` of the result (their source rows: ``xs``) against the CPU oracle, each row as its own sample carrying its
    row's scales."""
    S, stride, D = case["n_samples"], case["sample_stride"], 1 << case["log2d"]
    tidx = torch.from_numpy(idx).to(DEV)
    smp = (tidx // stride) % S
    wide = torch.float32 if got.dtype in FILL16 else got.dtype
    n = len(idx)
    if case["eye"]:
        xs = torch.zeros(n, D, device=DEV, dtype=wide)
        xs[torch.arange(n, device=DEV), tidx % case["group_rows"]] = \
            _per_row(case, c, case["c_ps"], tidx, smp).view(-1) if c is not None else 1.0
        cn = None
    else:
        xs = xs.to(wide)
        cn = None if c is None else _per_row(case, c, case["c_ps"], tidx, smp).expand(n, -1).cpu().numpy()
    an = None if a is None else _per_row(case, a, case["a_ps"], tidx, smp).expand(n, -1).cpu().numpy()
    bn = None if b is None else _per_row(case, b, True, tidx, smp).expand(n, -1).cpu().numpy()
    xs = xs.cpu().numpy()
    row_scales = case["axis"] == ft.AXIS_ROW or case["eye"]
    if case["one"]:        # a_s (.) FWHT(b_s (.) x): composed from the parts, as tests/test_streaming_parity_gpu.py does
        want = oracle.fwht(xs if bn is None else bn * xs)
        want = want if an is None else an * want
    else:
        want = oracle.pipeline(xs, an, bn, cn, n_samples=n, sample_stride=1, group_rows=1, axis="row" if row_scales else "col",
                               a_per_sample=an is not None, c_per_sample=cn is not None)
    want = torch.from_numpy(want).to(got.dtype)
    _same_bits(got[tidx].cpu(), want, (case["id"], "oracle rows"))


@pytest.mark.parametrize("index", range(len(ft.SPECS)), ids=[s["id"] for s in ft.SPECS])
def test_fused_case(index, hip_lib):
    cus = _cus()
    case = ft.sized(ft.SPECS[index], cus)
    la = ft.launch(case, cus)
    name, T = case["dtype"], DTYPE[case["dtype"]]
    rows, D = case["rows"], 1 << case["log2d"]
    assert ft.held_bytes(case) <= ft.MEMORY_CAP
    x, a, b, c = _operands(case, index)
    half = T in FILL16
    x32 = x.float() if half else None                          # the upcast input of the float32 reference launch
    oracle_idx = _oracle_rows(case, la)
    tidx = torch.from_numpy(oracle_idx).to(DEV)
    oracle_src = None if x is None else (x[tidx % case["sample_stride"]] if case["shared"] else x[tidx])
    buf, dst = _guard((rows, D), T)
    src = x
    if case["in_place"]:
        dst.copy_(x)
        src = dst
        if half:
            x = None                                           # (the upcast copy serves from here on: the memory cap)
    # ---- the launch and its symbol (the values come next: they do not rest on the plan query, which is checked last)
    before = None if x is None else int(_iview(x).sum())
    kernel = _launch(case, name, dst, src, a, b, c)
    SEEN.add(kernel)
    assert kernel == la.symbol == case["want_symbol"], (kernel, la.symbol)
    # ---- margins and coverage
    assert _margins_intact(buf, dst), "a byte outside the destination changed"
    assert _never_written(dst) == 0, "elements never written"
    assert x is None or int(_iview(x).sum()) == before, "the source is left alone"
    # ---- the whole output against the reference, a slab of rows at a time
    slab = max(1, ft.REF_SLAB_BYTES // (D * (4 if half else dst.element_size())))
    compared, unchanged = 0, 0
    if half:
        if case["in_place"]:                                   # before the reference launch overwrites the upcast input
            # A 16-bit format has too few values for y != x to hold on every element (two values of order one coincide about once
            # in 2^10 elements of float16, 2^7 of bfloat16).  A tile the launch never touched equals x on all of its elements:
            # no tile of the result may equal x on a sixteenth of them.
            te = 64 * ft.pick_k(name, case["log2d"]) * ft.vec(name)
            flat_y, flat_x, step = dst.view(-1), x32.view(-1), te * max(1, slab * D // te)
            for o in range(0, rows * D, step):
                eq = _iview(flat_y[o:o + step]) == _iview(flat_x[o:o + step].to(T))
                whole = eq.numel() // te * te
                assert whole == 0 or int(eq[:whole].view(-1, te).sum(1).max()) * 16 <= te, (case["id"], "a tile equals x")
                assert int(eq[whole:].sum()) * 16 <= max(16, eq.numel() - whole), (case["id"], "the last tile equals x")
        ref32 = x32 if case["in_place"] else torch.empty(rows, D, device=DEV, dtype=torch.float32)
        wide = _launch(case, "float", ref32, x32, a, b, c)
        assert wide.startswith("whvi::fused_shs_kernel<float, "), wide
    for r0 in range(0, rows, slab):
        r1 = min(rows, r0 + slab)
        want = ref32[r0:r1].to(T) if half else _chain(case, x, a, b, c, r0, r1)
        assert want.shape == (r1 - r0, D) and want.dtype == T
        _same_bits(dst[r0:r1], want, (case["id"], r0))
        compared += want.shape[0] * want.shape[1]
        if case["in_place"] and not half:
            unchanged += int((_iview(want) == _iview(x[r0:r1])).sum())
    assert compared == rows * D, "the whole output is compared"
    if case["in_place"] and not half:
        # y != x everywhere (but for the planted NaN and inf elements, whose own position may keep its bits): a tile the launch
        # never touched differs from the reference on every element
        assert unchanged <= 4, (case["id"], unchanged)
    # ---- rows against the CPU oracle
    _oracle_check(case, oracle_idx, dst, oracle_src, a, b, c)
    # ---- the plan query (the function the launch called) against the mirror, and the block map the case is there for
    c_null = c is None
    plan = _hip.fused_shs_plan(ft.DTYPE_CODE[name], rows, case["log2d"], case["n_samples"], case["sample_stride"], case["group_rows"],
                               ft.AXIS_ROW if case["eye"] else case["axis"], ft.flags_of(case), case["in_place"], case["eye"],
                               c_null, 0)
    assert plan == (0, la.stage, int(la.nt), la.mode, la.grid), (plan, la)
    assert plan == _hip.fused_shs_plan(ft.DTYPE_CODE[name], rows, case["log2d"], case["n_samples"], case["sample_stride"],
                                       case["group_rows"], ft.AXIS_ROW if case["eye"] else case["axis"], ft.flags_of(case),
                                       case["in_place"], case["eye"], c_null, cus)
    assert ft.block_map(bool(plan[2]), plan[4], plan[3]) == case["want_map"], (case["id"], plan)


def test_every_shipped_symbol_was_launched(hip_lib):
    """The union of the symbols whvi_last_kernel reported above is the fused forward's shipped set (the mirror's statement of
    it, which tests/test_fused_table_host.py holds against the library) minus the documented unreachable ones."""
    for index, spec in enumerate(ft.SPECS):                    # run on its own, this test launches the cases itself
        if spec["want_symbol"] not in SEEN:
            test_fused_case(index, hip_lib)
    assert sorted(ft.shipped() - set(ft.UNREACHABLE) - SEEN) == [], "shipped and reachable, but no case of this run launched it"
    assert sorted(SEEN - ft.shipped()) == []
