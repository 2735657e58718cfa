"""GPU parity of the fused pipeline on 16-bit activation streams (``whvi_fused_shs_ex_f16 / _bf16``).

Contract (include/whvi_hip.h): on every element

    fused_shs(x16, a, b, c, ...) == fused_shs(x16.float(), a, b, c, ...).to(x16.dtype)

-- the float32 pipeline on the exactly-upcast input, rounded ONCE.  The arbiter is ``oracle.pipeline(axis="col")`` on the
upcast input followed by torch's round-to-nearest-even cast (the construction tests/test_fwht_gpu.py uses for the 16-bit
transform).  Values equal, NaN positions identical, no tolerance; the sign of an exact zero is exempt as far as the header
exempts it for the f32 fused kernel, so both sides are compared after ``+ 0.0``."""
import numpy as np
import pytest
import torch

import oracle
from whvi_amd import _hip
from whvi_amd.fastfood import FastfoodFunction, WHVIFastfoodMatrix

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
KERNEL = "fused_shs16_kernel"


def _np(v):
    return None if v is None else v.detach().float().cpu().numpy()


def _want(x16, a, b, c, **kw):
    """The arbiter: oracle pipeline in float32 on the upcast input, one RNE cast."""
    y = oracle.pipeline(x16.float().cpu().numpy(), _np(a), _np(b), _np(c), axis="col", **kw)
    return torch.from_numpy(y).to(x16.dtype)


def _assert_same(got, want, what):
    g, w = got.detach().cpu().float() + 0.0, want.detach().cpu().float() + 0.0
    gn, wn = torch.isnan(g), torch.isnan(w)
    assert torch.equal(gn, wn), (what, "NaN positions differ", int((gn != wn).sum()))
    bad = (g != w) & ~gn
    assert not bool(bad.any()), (what, int(bad.sum()), "first", g[bad][:4].tolist(), w[bad][:4].tolist())
    assert torch.equal(torch.isinf(g), torch.isinf(w)), what


def _vectors(g, S, d, scale):
    a = torch.randn(d, generator=g) * scale
    b = torch.randn(S, d, generator=g) * scale
    c = torch.randn(d, generator=g)
    return a.to(DEV), b.to(DEV), c.to(DEV)


# (rows, n_samples, sample_stride): ragged last tiles and idle waves (1, 3, 257, 12345 rows); one, three and 64 samples with
# a sample_stride that divides the rows of a block (powers of two) and one that does not (3, 5, 193)
SHAPES = [(1, 1, 1), (3, 3, 1), (257, 3, 5), (257, 64, 4), (257, 1, 7), (12345, 64, 193), (12345, 3, 4096), (64, 64, 1)]


@pytest.mark.parametrize("log2d", list(range(3, 14)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_at_every_size(dtype, log2d, hip_lib):
    d = 1 << log2d
    g = torch.Generator().manual_seed(100 + log2d)
    scale = 1.0 / d ** 0.5                                    # results of order one: finite in fp16
    for rows, S, stride in SHAPES:
        if rows * d > (1 << 24) and (S, stride) != (64, 193):
            continue                                          # the largest row count once per row length is enough
        x = torch.randn(rows, d, generator=g).to(dtype).to(DEV)
        a, b, c = _vectors(g, S, d, scale)
        want = _want(x, a, b, c, n_samples=S, sample_stride=stride)
        got = _hip.fused_shs(x, a, b, c, n_samples=S, sample_stride=stride)              # out of place
        assert got.dtype == dtype and KERNEL in _hip.last_kernel(), _hip.last_kernel()
        _assert_same(got, want, (dtype, log2d, rows, S, stride, "out of place"))
        y = x.clone()
        assert _hip.fused_shs(y, a, b, c, n_samples=S, sample_stride=stride, out=y) is y  # in place
        _assert_same(y, want, (dtype, log2d, rows, S, stride, "in place"))


@pytest.mark.parametrize("log2d", [3, 6, 9, 11, 13])
@pytest.mark.parametrize("dtype", DTYPES)
def test_absent_vectors_and_per_sample_outer_vectors(dtype, log2d, hip_lib):
    d, rows, S, stride = 1 << log2d, 131, 3, 5
    g = torch.Generator().manual_seed(7 + log2d)
    x = torch.randn(rows, d, generator=g).to(dtype).to(DEV)
    a, b, c = _vectors(g, S, d, 1.0 / d ** 0.5)
    for drop in ("a", "b", "c", "abc"):
        va, vb, vc = (None if "a" in drop else a), (None if "b" in drop else b), (None if "c" in drop else c)
        got = _hip.fused_shs(x, va, vb, vc, n_samples=S, sample_stride=stride)
        _assert_same(got, _want(x, va, vb, vc, n_samples=S, sample_stride=stride), (dtype, log2d, "without", drop))
    aS, cS = torch.randn(S, d, generator=g).to(DEV) / d ** 0.5, torch.randn(S, d, generator=g).to(DEV)
    for aps, cps in ((True, False), (False, True), (True, True)):
        va, vc = (aS if aps else a), (cS if cps else c)
        got = _hip.fused_shs(x, va, b, vc, n_samples=S, sample_stride=stride, a_per_sample=aps, c_per_sample=cps)
        want = _want(x, va, b, vc, n_samples=S, sample_stride=stride, a_per_sample=aps, c_per_sample=cps)
        _assert_same(got, want, (dtype, log2d, "per-sample", aps, cps))


def _sampled_rows_check(x, y, keep, a, b, c, S, stride, aps, cps, what):
    """Rows ``keep`` of a large launch against the oracle: each kept row becomes its own "sample" carrying the vectors of the
    sample it belongs to in the launch."""
    keep = sorted(set(int(k) for k in keep))
    s = torch.tensor([(k // stride) % S for k in keep])
    va = a[s.to(a.device)] if aps else a
    vc = c[s.to(c.device)] if cps else c
    vb = b[s.to(b.device)]
    want = _want(x[keep], va, vb, vc, n_samples=len(keep), sample_stride=1, a_per_sample=aps, c_per_sample=cps)
    _assert_same(y[keep], want, what)


# which launch form a shape selects (whvi_amd/csrc/dispatch.hpp): every row of a block in one sample -> a, b, c staged in LDS
# (a and c alone at D = 8192); shared a / c otherwise -> a, c staged; per-sample a / c otherwise -> every vector from L2
LARGE = [(5, "from_l2")] + [(k, f) for k in (9, 11, 12, 13) for f in ("one_sample_blocks", "shared_ac", "from_l2")]


@pytest.mark.parametrize("mib", [320, 96])
@pytest.mark.parametrize("log2d,form", LARGE)
@pytest.mark.parametrize("dtype", DTYPES)
def test_large_launches_sampled_rows(dtype, log2d, form, mib, hip_lib):
    """320 MiB in place is the streaming instantiation (non-temporal loads, write-through stores, XCD-contiguous block order,
    store barrier), 96 MiB the cache-resident launch that fills the chip; a row count that is not a multiple of 8 as well.
    (Sampled rows at the timed sizes; tests/test_fused_table_gpu.py compares the whole output of every instantiation, on
    every block map, at the smallest shape of each regime.)"""
    d, S = 1 << log2d, 64
    nt = mib > 256
    for extra in (0, 3):
        rows = (mib << 20) // (2 * d) + extra
        stride = 4096 if form == "one_sample_blocks" else 4099
        aps = cps = form == "from_l2"
        gen = torch.Generator(device=DEV).manual_seed(31 * log2d + extra)
        x = torch.randn(rows, d, device=DEV, generator=gen).to(dtype)
        a = torch.randn((S, d) if aps else (d,), device=DEV, generator=gen) / d ** 0.5
        c = torch.randn((S, d) if cps else (d,), device=DEV, generator=gen)
        b = torch.randn(S, d, device=DEV, generator=gen) / d ** 0.5
        y = x.clone()
        _hip.fused_shs(y, a, b, c, n_samples=S, sample_stride=stride, a_per_sample=aps, c_per_sample=cps, out=y)
        name = _hip.last_kernel()
        stage = 0 if (log2d < 9 or form == "from_l2") else (1 if (form == "shared_ac" or log2d == 13) else 3)
        assert name.startswith(f"whvi::{KERNEL}<") and name.endswith(f"{'true' if nt else 'false'}, 0, {stage}, 256>"), name
        pick = torch.randint(0, rows, (24,), generator=torch.Generator().manual_seed(rows)).tolist()
        keep = [0, 1, 7, 8, stride - 1, stride, stride + 1, rows // 2, rows - 9, rows - 8, rows - 2, rows - 1] + pick
        _sampled_rows_check(x, y, keep, a, b, c, S, stride, aps, cps, (dtype, log2d, mib, form, rows))
        del x, y


@pytest.mark.parametrize("log2d", [3, 7, 10, 13])
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values(dtype, log2d, hip_lib):
    """Subnormals, signed zeros, the largest finite values, infinities and NaN in the input; 0, inf and NaN in the scale
    vectors; fp16 overflow to inf where the single rounding puts it."""
    d, rows, S = 1 << log2d, 40, 2
    fi = torch.finfo(dtype)
    g = torch.Generator().manual_seed(log2d)
    x = torch.randn(rows, d, generator=g).to(dtype)
    specials = torch.tensor([0.0, -0.0, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.tiny / 4, float("inf"), float("-inf"),
                             float("nan"), fi.max / 2, 1.0], dtype=torch.float32).to(dtype)
    for r in range(rows):
        kind = r % 5
        if kind == 0:
            continue                                           # plain Gaussian rows between the special ones
        idx = torch.randint(0, d, (max(1, d // 8),), generator=g)
        lim = {1: 7, 2: 9, 3: 12, 4: 10}[kind]                 # finite specials only / + inf / everything / + NaN without inf
        vals = specials[torch.randint(0, lim, (idx.numel(),), generator=g)]
        if kind == 4:
            vals = torch.where(torch.isinf(vals), torch.zeros_like(vals), vals)
        x[r, idx] = vals
    x[5] = 0.0
    x[6] = -0.0
    x[7] = fi.max                                              # overflows the 16-bit range after the first transform
    x = x.to(DEV)
    a, b, c = _vectors(g, S, d, 1.0 / d ** 0.5)
    for variant in range(4):
        va, vb, vc = a.clone(), b.clone(), c.clone()
        if variant >= 1:
            vc[1], va[2], vb[0, 3], vb[1, 0] = 0.0, 0.0, 0.0, -0.0
        if variant >= 2:
            vc[4], va[5 % d], vb[1, 6 % d] = float("inf"), float("-inf"), float("inf")
        if variant >= 3:
            vc[7 % d], va[0], vb[0, 2] = float("nan"), float("nan"), float("nan")
        got = _hip.fused_shs(x, va, vb, vc, n_samples=S, sample_stride=3)
        want = _want(x, va, vb, vc, n_samples=S, sample_stride=3)
        _assert_same(got, want, (dtype, log2d, "variant", variant))
    if dtype == torch.float16:                                 # large but finite in f32, beyond fp16: +-inf from the one rounding
        big = _hip.fused_shs(x, None, None, None)
        want = _want(x, None, None, None)
        assert bool(torch.isinf(want[7]).any()) or d < 64
        _assert_same(big, want, (dtype, log2d, "overflow"))


ONE_ROUNDING_SEED = 2024


def one_rounding_case(dtype, seed=ONE_ROUNDING_SEED, d=4096, rows=96, S=3):
    """Inputs of the one-rounding comparison, all exactly representable in ``dtype``, and the float64 pipeline on them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, d, generator=g).to(dtype)
    a = (torch.randn(d, generator=g) / d ** 0.5).to(dtype)
    b = (torch.randn(S, d, generator=g) / d ** 0.5).to(dtype)
    c = torch.randn(d, generator=g).to(dtype)
    ref = oracle.pipeline(x.double().numpy(), a.double().numpy(), b.double().numpy(), c.double().numpy(), n_samples=S,
                          sample_stride=rows // S, axis="col")
    return x, a, b, c, torch.from_numpy(ref), rows // S


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_rounding_not_five(dtype, hip_lib):
    """Seeded Gaussian rows at D = 4096, judged in float64: the launch (one rounding) is no further from the float64 pipeline
    of the same 16-bit inputs than the unfused 16-bit chain (three multiplies and two transforms, five roundings), in the
    largest elementwise error and in RMS, and strictly closer in RMS."""
    x, a, b, c, ref, stride = one_rounding_case(dtype)
    S, rows = b.shape[0], x.shape[0]
    xd, ad, bd, cd = (t.to(DEV) for t in (x, a, b, c))
    fused = _hip.fused_shs(xd, ad.float(), bd.float(), cd.float(), n_samples=S, sample_stride=stride)
    assert fused.dtype == dtype
    rix = (torch.arange(rows, device=DEV) // stride) % S
    chain = ad * _hip.fwht_rows(bd[rix] * _hip.fwht_rows(cd * xd))
    assert chain.dtype == dtype
    err_f = fused.cpu().double() - ref
    err_c = chain.cpu().double() - ref
    assert torch.isfinite(err_f).all() and torch.isfinite(err_c).all()
    max_f, max_c = float(err_f.abs().max()), float(err_c.abs().max())
    rms_f, rms_c = float(err_f.pow(2).mean().sqrt()), float(err_c.pow(2).mean().sqrt())
    print(f"one rounding vs five, {dtype}: max {max_f:.4e} vs {max_c:.4e}, rms {rms_f:.4e} vs {rms_c:.4e}")
    assert max_f <= max_c and rms_f <= rms_c and rms_f < rms_c, (max_f, max_c, rms_f, rms_c)


@pytest.mark.parametrize("dtype", DTYPES)
def test_refused_forms_raise_and_f32_f64_still_run(dtype, hip_lib):
    d, rows, S = 512, 8, 2
    g = torch.Generator().manual_seed(3)
    x16 = torch.randn(rows, d, generator=g).to(dtype).to(DEV)
    a, b, c = _vectors(g, S, d, 1.0)
    calls = {
        "axis='row'": lambda x, k: _hip.fused_shs(x, k(a[:rows]), k(b[:, :rows]), k(c[:rows]), axis="row", n_samples=S,
                                                   group_rows=rows),
        "src=None": lambda x, k: _hip.fused_shs(None, None, k(b), k(c), axis="row", n_samples=S, group_rows=d, rows=S * d, d=d,
                                                 sample_stride=d, dtype=x.dtype, device=x.device),
        "src_shared": lambda x, k: _hip.fused_shs(x[:4], k(a), k(b), None, n_samples=S, sample_stride=4, src_shared=True),
        "one_transform": lambda x, k: _hip.fused_shs(x, k(a), k(b), None, n_samples=S, one_transform=True),
    }
    for form, call in calls.items():
        with pytest.raises(RuntimeError) as e:
            call(x16, lambda v: v)
        assert form in str(e.value), (form, str(e.value))
        for wide in (torch.float32, torch.float64):
            out = call(x16.to(wide), lambda v: v.to(wide))
            assert out.dtype == wide and bool(torch.isfinite(out).all())
    # the C entry itself refuses them as well (device pointers, no launch)
    fn = getattr(_hip.lib(), "whvi_fused_shs_ex_" + ("f16" if dtype == torch.float16 else "bf16"))
    y = torch.empty_like(x16)
    for axis, src, flags, word in ((0, x16.data_ptr(), 0, "row-axis"), (1, None, 0, "identity-source"),
                                   (1, x16.data_ptr(), 4, "shared-source"), (1, x16.data_ptr(), 8, "one-transform")):
        rc = fn(y.data_ptr(), src, None, None, None, rows, 9, 1, 1, 1, axis, flags, None)
        assert rc in (-1, -2) and word in _hip.last_error(), (rc, _hip.last_error())


def _layer(d, bias=False):
    torch.manual_seed(11)
    layer = WHVIFastfoodMatrix(d, bias=bias).to(DEV)
    with torch.no_grad():
        layer.s1.mul_(30.0)
        layer.s2.mul_(30.0)
        layer.g_mu.normal_()
        if bias:
            layer.bias.normal_()
    return layer


@pytest.mark.parametrize("d", [64, 2048])
@pytest.mark.parametrize("dtype", DTYPES)
def test_module_keep_half_forward(dtype, d, hip_lib, monkeypatch):
    S, B = 3, 10
    layer = _layer(d)
    x = torch.randn(S, B, d, generator=torch.Generator().manual_seed(5)).to(dtype).to(DEV)
    # flag off (the default): float32 out, bit-equal to the promoted composition of separate launches, spelled out
    assert WHVIFastfoodMatrix.keep_half is False
    torch.manual_seed(77)
    off = layer.forward_mc(x, S)
    torch.manual_seed(77)
    eps = torch.randn(S, d, device=DEV)
    gk = layer.g_mu + torch.nn.functional.softplus(layer.g_rho) * eps
    flat = x.reshape(S * B, d)
    rix = torch.arange(S * B, device=DEV) // B % S
    spelled = layer.s1 * _hip.fwht_rows(gk[rix] * _hip.fwht_rows(layer.s2 * flat))
    assert off.dtype == torch.float32 and spelled.dtype == torch.float32
    assert torch.equal(off.detach().reshape(S * B, d).view(torch.int32), spelled.detach().view(torch.int32))
    # flag on: one 16-bit launch, the input's dtype, equal to the float32 layer on the upcast input cast once
    monkeypatch.setattr(layer, "keep_half", True, raising=False)
    torch.manual_seed(77)
    on = layer.forward_mc(x, S)
    assert on.dtype == dtype and on.shape == (S, B, d) and KERNEL in _hip.last_kernel()
    torch.manual_seed(77)
    wide = layer.forward_mc(x.float(), S)
    assert wide.dtype == torch.float32
    _assert_same(on, wide.to(dtype), (dtype, d, "keep_half forward"))
    # a (batch, D) input shared by all samples is expanded; the bias is added in the activation's dtype
    biased = _layer(d, bias=True)
    biased.keep_half = True
    torch.manual_seed(78)
    got = biased.forward_mc(x[0], S)
    torch.manual_seed(78)
    plain16 = _hip.fused_shs(x[0].repeat(S, 1), biased.s1.detach(), _g(biased, 78, S, d), biased.s2.detach(), n_samples=S,
                             sample_stride=B)
    assert got.dtype == dtype and got.shape == (S, B, d)
    _assert_same(got, plain16.view(S, B, d) + biased.bias.detach().to(dtype), (dtype, d, "shared input + bias"))


def _g(layer, seed, S, d):
    torch.manual_seed(seed)
    eps = torch.randn(S, d, device=DEV)
    return (layer.g_mu + layer.g_sigma * eps).detach()


@pytest.mark.parametrize("d", [64, 2048])
@pytest.mark.parametrize("dtype", DTYPES)
def test_module_keep_half_backward(dtype, d, hip_lib, monkeypatch):
    S, B = 3, 6
    g = torch.Generator().manual_seed(9)
    x16 = torch.randn(S * B, d, generator=g).to(dtype).to(DEV)
    w16 = torch.randn(S * B, d, generator=g).to(dtype).to(DEV)
    a, b, c = _vectors(g, S, d, 1.0 / d ** 0.5)
    # float32 FastfoodFunction on the upcast inputs
    x32 = x16.float().requires_grad_(True)
    p32 = [t.clone().requires_grad_(True) for t in (a, b, c)]
    y32 = FastfoodFunction.apply(x32, *p32, S, B)
    ref = torch.autograd.grad(y32, [x32] + p32, grad_outputs=w16.float())
    # keep_half with parameter gradients: x and grad_y upcast once, float32 code, grad_x cast once
    xh = x16.clone().requires_grad_(True)
    ph = [t.clone().requires_grad_(True) for t in (a, b, c)]
    yh = FastfoodFunction.apply(xh, *ph, S, B, False, True)
    assert yh.dtype == dtype and KERNEL in _hip.last_kernel()
    _assert_same(yh, y32.to(dtype), (dtype, d, "forward"))
    got = torch.autograd.grad(yh, [xh] + ph, grad_outputs=w16)
    assert got[0].dtype == dtype and all(t.dtype == torch.float32 for t in got[1:])
    _assert_same(got[0], ref[0].to(dtype), (dtype, d, "grad_x"))
    for name, gg, rr in zip("abc", got[1:], ref[1:]):
        assert torch.equal(gg.view(torch.int32), rr.view(torch.int32)), (dtype, d, "grad_" + name)
    # grad_x alone: ONE 16-bit launch, a and c exchanged
    xo = x16.clone().requires_grad_(True)
    yo = FastfoodFunction.apply(xo, a, b, c, S, B, False, True)
    launches = []                                             # (the backward runs on autograd's thread; last_kernel() is per thread)
    real_fused, real_fwht = _hip.fused_shs, _hip.fwht_rows

    def spy_fused(*args, **kw):
        out = real_fused(*args, **kw)
        launches.append(_hip.last_kernel())
        return out

    def spy_fwht(*args, **kw):
        out = real_fwht(*args, **kw)
        launches.append(_hip.last_kernel())
        return out

    monkeypatch.setattr(_hip, "fused_shs", spy_fused)
    monkeypatch.setattr(_hip, "fwht_rows", spy_fwht)
    (gx,) = torch.autograd.grad(yo, [xo], grad_outputs=w16)
    monkeypatch.undo()
    assert len(launches) == 1 and KERNEL in launches[0], launches
    assert gx.dtype == dtype
    _assert_same(gx, ref[0].to(dtype), (dtype, d, "grad_x alone"))
    direct = _hip.fused_shs(w16, c, b, a, n_samples=S, sample_stride=B)
    _assert_same(gx, direct, (dtype, d, "grad_x alone is the launch with a and c exchanged"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_hip_graph_replay(dtype, hip_lib):
    d, rows, S = 2048, 24, 3
    g = torch.Generator().manual_seed(4)
    x = torch.randn(rows, d, generator=g).to(dtype).to(DEV)
    a, b, c = _vectors(g, S, d, 1.0 / d ** 0.5)
    eager = _hip.fused_shs(x, a, b, c, n_samples=S, sample_stride=8)
    y = torch.zeros_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _hip.fused_shs(x, a, b, c, n_samples=S, sample_stride=8, out=y)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _hip.fused_shs(x, a, b, c, n_samples=S, sample_stride=8, out=y)
    for _ in range(3):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int16), eager.view(torch.int16))
