"""The one-launch stacked diagonal route (whvi_diag_apply_stacked_f32, ``WHVIStackedMatrix.diag_blocks``) without a GPU: the C
ABI is declared and exported, every argument check answers before any HIP call, the support rule is mirrored in Python, the
opt-in changes nothing on host tensors, survives copies and pickles and leaves the checkpoint keys alone, the case table
meets every switch at every row length, and the shipped kernels use no scratch."""
import copy
import ctypes
import os
import pickle
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ERR_ARG, ERR_SIZE, ERR_ALIGN, ERR_OVERLAP = -1, -2, -3, -5


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "whvi_hip.h")).read()
    assert "int whvi_diag_apply_stacked_supported(int32_t log2d, int64_t n_blocks);" in header
    assert "int whvi_diag_apply_stacked_f32(void *out, const void *x, const void *s1, const void *s2, const void *u" in header
    from whvi_amd import _hip
    L = _hip.lib()
    assert hasattr(L, "whvi_diag_apply_stacked_f32") and hasattr(L, "whvi_diag_apply_stacked_supported")


def test_argument_checks_without_gpu():
    from whvi_amd import _hip
    L = _hip.lib()
    buf = (ctypes.c_char * (1 << 16))()
    p = (ctypes.addressof(buf) + 15) & ~15
    out, x, s1, s2, u, bias = (p + 8192 * i for i in range(6))
    f = L.whvi_diag_apply_stacked_f32

    def call(out=out, x=x, s1=s1, s2=s2, u=u, bias=None, S=2, B=3, log2d=4, J=2, n_cols=20, ld_out=24, flags=2):
        return f(out, x, s1, s2, u, bias, S, B, log2d, J, n_cols, ld_out, flags, None)

    # (none of these launches: a launch on this host would answer WHVI_ERR_LAUNCH = -4, which no check below accepts)
    for bad in (dict(S=-1), dict(B=-1), dict(J=-1), dict(n_cols=-1), dict(ld_out=-1)):
        assert call(**bad) == ERR_ARG and "negative" in _hip.last_error(), bad
    assert call(flags=64) == ERR_ARG and "unknown flags" in _hip.last_error()          # (the plain-order tuning flag: not here)
    assert call(flags=256) == ERR_ARG and "unknown flags" in _hip.last_error()
    assert call(log2d=1) == ERR_SIZE and "log2(D)" in _hip.last_error()
    assert call(log2d=13) == ERR_SIZE and "log2(D)" in _hip.last_error()
    assert call(J=0) == ERR_SIZE and "n_blocks" in _hip.last_error()
    assert call(J=513, n_cols=1, ld_out=1) == ERR_SIZE and "LDS" in _hip.last_error()      # 8 * 513 * 16 > 65536
    assert call(log2d=12, J=3, n_cols=1, ld_out=1) == ERR_SIZE and "LDS" in _hip.last_error()
    assert call(n_cols=0) == ERR_ARG and "n_cols" in _hip.last_error()
    assert call(n_cols=33, ld_out=40) == ERR_ARG and "n_cols" in _hip.last_error()         # J D = 32
    assert call(n_cols=20, ld_out=19) == ERR_ARG and "ld_out" in _hip.last_error()
    assert call(S=0) == 0 and _hip.last_error() == ""                                      # nothing to do: no launch
    assert call(B=0, out=None, x=None) == 0 and _hip.last_error() == ""
    assert call(S=1 << 16, B=1 << 16) == ERR_SIZE and "32 bits" in _hip.last_error()
    assert call(S=1 << 40, B=1 << 40) == ERR_SIZE and "32 bits" in _hip.last_error()       # (the product overflows 64 bits)
    for name in ("out", "x", "s1", "s2", "u"):
        assert call(**{name: None}) == ERR_ARG and "null pointer" in _hip.last_error(), name
    for name in ("x", "s1", "s2", "u", "bias"):
        assert call(**{name: locals()[name] + 4}) == ERR_ALIGN and "aligned" in _hip.last_error(), name
    assert call(out=out + 2) == ERR_ALIGN and "aligned" in _hip.last_error()
    # out: S B = 6 rows at pitch 24, 20 columns of the last one = 140 floats = 560 bytes
    assert call(out=x) == ERR_OVERLAP and "overlaps" in _hip.last_error()                  # in-place use
    assert call(out=x - 544) == ERR_OVERLAP                                                # the last 16 bytes written are x's first
    assert call(out=u - 560 + 16, flags=2) == ERR_OVERLAP
    assert call(out=s1 + 64) == ERR_OVERLAP and call(out=s2 - 16) == ERR_OVERLAP
    assert call(out=bias + 112, bias=bias) == ERR_OVERLAP                                  # bias: J D = 32 floats = 128 bytes
    assert call(out=x + 176, flags=2 | 1) == ERR_OVERLAP                                   # a shared x is B D floats = 192 bytes
    assert call(out=x + 368, flags=2) == ERR_OVERLAP                                       # a per-sample one S B D = 384


def test_supported_rule_is_mirrored_in_python():
    from whvi_amd import _hip
    L = _hip.lib()
    for log2d in range(0, 14):
        for J in range(1, 601):
            want = bool(L.whvi_diag_apply_stacked_supported(log2d, J))
            assert _hip.diag_apply_stacked_supported(torch.float32, 1 << log2d, J) == want, (log2d, J)
    assert not L.whvi_diag_apply_stacked_supported(4, 0) and not _hip.diag_apply_stacked_supported(torch.float32, 16, 0)
    assert not _hip.diag_apply_stacked_supported(torch.float64, 16, 1)
    # the shapes the issue names: D = 16 .. 2048 with J D <= 4096, D = 4 and 8, the widest row, the edge of the LDS rule
    for d in (16, 128, 1024, 2048):
        assert _hip.diag_apply_stacked_supported(torch.float32, d, 4096 // d)
    assert _hip.diag_apply_stacked_supported(torch.float32, 4, 16) and _hip.diag_apply_stacked_supported(torch.float32, 8, 128)
    assert _hip.diag_apply_stacked_supported(torch.float32, 4096, 2) and not _hip.diag_apply_stacked_supported(torch.float32, 4096, 3)


def _layer(n_in, n_out, bias=True, flag=False, seed=3):
    from whvi_amd.weights import WHVIStackedMatrix
    torch.manual_seed(seed)
    layer = WHVIStackedMatrix(n_in, n_out, bias=bias)
    layer.diag_blocks = flag
    return layer


def _net(n_in, flag):
    from whvi_amd.layers import WHVILinear
    from whvi_amd.networks import WHVIRegression
    torch.manual_seed(5)
    net = WHVIRegression([WHVILinear(n_in, 128, bias=True), nn.ReLU(), WHVILinear(128, 128, bias=True), nn.ReLU(),
                          WHVILinear(128, 2, bias=True)], train_samples=3)
    return net.set_stacked_diagonal(flag)


def test_flag_is_a_class_default_and_the_network_sets_it():
    from whvi_amd.weights import WHVIStackedMatrix
    assert WHVIStackedMatrix.diag_blocks is False
    net = _net(16, False)
    stacked = [m for m in net.modules() if isinstance(m, WHVIStackedMatrix)]
    assert len(stacked) == 2 and not any(m.diag_blocks for m in stacked)
    assert net.set_stacked_diagonal() is net and all(m.diag_blocks for m in stacked)
    net.set_stacked_diagonal(False)
    assert not any(m.diag_blocks for m in stacked)
    # host tensors never take the route, whatever the flag says; nor does a layer whose hip_apply is off (faithful dataflow)
    layer = _layer(16, 128, flag=True)
    assert not layer._diag_blocks_route(torch.randn(5, 16)) and not layer.fuses_relu(torch.randn(5, 16))


def test_flag_changes_nothing_on_host_tensors():
    x = torch.randn(9, 16)
    outs = []
    for flag in (False, True):
        layer = _layer(16, 130, flag=flag)
        torch.manual_seed(11)
        one = layer(x)
        mc = layer.forward_mc(x, 3, relu_in=True, relu_out=True)
        mc3 = layer.forward_mc(torch.randn(3, 9, 16), 3)
        outs.append((one, mc, mc3, layer.kl))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    losses = []
    for flag in (False, True):
        net = _net(8, flag)
        torch.manual_seed(13)
        xb, yb = torch.randn(7, 8), torch.randn(7, 2)
        loss = net.loss(xb, yb, n=100)
        loss.backward()
        losses.append((loss.detach(), [p.grad.clone() for p in net.parameters()]))
    assert torch.equal(losses[0][0], losses[1][0])
    assert all(torch.equal(a, b) for a, b in zip(losses[0][1], losses[1][1]))


def test_copies_and_pickles_keep_the_flag_and_the_state_dict_keys_do_not_change():
    plain, flagged = _layer(16, 130, flag=False), _layer(16, 130, flag=True)
    assert list(plain.state_dict().keys()) == list(flagged.state_dict().keys())
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), flagged.state_dict().values()))
    for clone in (copy.deepcopy(flagged), pickle.loads(pickle.dumps(flagged))):
        assert clone.diag_blocks is True and list(clone.state_dict().keys()) == list(plain.state_dict().keys())
    assert copy.deepcopy(plain).diag_blocks is False
    packed = _layer(16, 130, flag=True).pack_parameters()
    assert list(packed.state_dict().keys()) == list(plain.state_dict().keys())
    clone = pickle.loads(pickle.dumps(packed))
    assert clone.diag_blocks is True and clone._packed and [n for n, _ in clone.named_parameters()] == [n for n, _ in packed.named_parameters()]
    net = _net(16, True)
    assert list(net.state_dict().keys()) == list(_net(16, False).state_dict().keys())
    assert all(m.diag_blocks for m in copy.deepcopy(net).modules() if hasattr(type(m), "diag_blocks"))


def test_backward_ops_match_float64_autograd_of_the_expression():
    """``StackedDiagApplyFunction.backward`` is torch ops only, so it is checked here, on the host, against float64 autograd of
    ``_reference_ops`` -- full blocks plus a ragged one, both ReLUs, a bias, shared and per-sample x."""
    from whvi_amd.weights import StackedDiagApplyFunction as F_

    class Ctx:
        pass

    g = torch.Generator().manual_seed(2)
    J, D, S, B = 3, 8, 2, 5
    for n_cols, shared, mean_plus in ((21, False, True), (24, True, True), (2, False, False), (8, True, False)):
        x = torch.randn((B, D) if shared else (S, B, D), generator=g)
        s1, s2 = torch.randn(J, D, generator=g), torch.randn(J, D, generator=g)
        u, bias = torch.randn(J, S + (1 if mean_plus else 0), D, generator=g), torch.randn(1, J * D, generator=g)
        go = torch.randn(S, B, n_cols, generator=g)
        ops64 = [t.double().requires_grad_() for t in (x, s1, s2, u, bias)]
        out64 = F_._reference_ops(*ops64[:4], ops64[4], n_cols, mean_plus, True, True)
        want = torch.autograd.grad(out64, ops64, go.double())
        ctx = Ctx()
        ctx.n_samples, ctx.n_cols, ctx.mean_plus, ctx.relu_in, ctx.relu_out = S, n_cols, mean_plus, True, True
        ctx.bias_shape, ctx.needs_input_grad = (1, J * D), (True,) * 5
        ctx.saved_tensors = (x, s1, s2, u, out64.float())
        got = F_.backward(ctx, go)[:5]
        for a, b in zip(got, want):
            assert a.shape == b.shape
            assert float((a.double() - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-30, (n_cols, shared)


def test_case_table_meets_every_switch_at_every_row_length():
    import stacked_diag_cases as sc
    from whvi_amd import _hip
    assert set(sc.DIMS) >= {4, 16, 64, 128, 256, 1024, 4096}
    for D in sc.DIMS:
        cases = [c for c in sc.CASES if c.D == D and not c.tune]
        for field in ("S", "shared", "bias", "relu_in", "relu_out", "mean_plus"):
            assert len({getattr(c, field) for c in cases}) == 2, (D, field)
        assert {c.B for c in cases} == ({1, 37, 259} if D <= 256 else {1, 37})
        geoms = {(c.J, c.n_cols, c.ld_out) for c in cases}
        assert {(1, 2, 2), (1, 2, 8), (1, D, D)} <= geoms and len(geoms) >= 6
        # both lane maps of the short rows: fewer blocks than lane groups per wave (256 / D), and at least as many
        if D < 256:
            assert any(J < 256 // D for J, _, _ in geoms) and any(J >= 256 // D for J, _, _ in geoms), D
        assert any(ld == n and n % 4 for _, n, ld in geoms) and any(ld > n and J > 1 for J, n, ld in geoms)
    for c in sc.CASES + (sc.STREAM_CASE,):
        assert _hip.diag_apply_stacked_supported(torch.float32, c.D, c.J) and 1 <= c.n_cols <= c.J * c.D <= c.ld_out + c.J * c.D
        assert c.ld_out >= c.n_cols
    assert len({sc.case_id(c) for c in sc.CASES}) == len(sc.CASES)
    s = sc.STREAM_CASE
    assert 4 * s.S * s.B * s.n_cols > 256 << 20 and 4 * s.S * (s.B - 100) * s.n_cols <= 256 << 20      # just over the threshold


def test_shipped_library_holds_the_kernels_without_scratch():
    from shipped_isa import ShippedLibrary
    with ShippedLibrary() as lib:
        found = {n: k for n, k in lib.kernels.items() if n.startswith("whvi::diag_apply_stacked_kernel<")}
        for c in (1, 2, 4, 8, 16):
            for nt in ("false", "true"):
                k = lib.find(f"whvi::diag_apply_stacked_kernel<float, {c}, {nt}>")
                assert k["scratch"] == 0 and k["lds"] == 0, (c, nt, k)          # (the diagonals live in dynamic LDS)
                # at least two waves per SIMD (512 registers per lane and SIMD) at every row length
                assert k["vgprs"] + k["agprs"] <= 256, (c, nt, k["vgprs"], k["agprs"])
        assert len(found) == 10
