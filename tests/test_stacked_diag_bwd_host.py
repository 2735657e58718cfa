"""The one-launch backward of the stacked diagonal route (whvi_diag_apply_stacked_bwd_f32,
``WHVIStackedMatrix.diag_blocks_backward``) without a GPU: the C ABI is declared and exported, every argument check answers
before any HIP call, both support rules agree, the slab count is deterministic, the opt-in changes nothing on host tensors,
survives copies and pickles and leaves the checkpoint keys alone, the torch ops the flag-on Function falls back to match
float64 autograd, the case table meets every switch at every row length, and the shipped kernels use no scratch."""
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
    assert "int whvi_diag_apply_stacked_bwd_supported(int32_t log2d, int64_t n_blocks);" in header
    assert "int64_t whvi_diag_apply_stacked_bwd_slabs(int64_t S, int64_t B, int32_t log2d, int64_t n_blocks, int64_t n_cols);" in header
    assert "int whvi_diag_apply_stacked_bwd_f32(void *grad_x, void *out, void *part, const void *g, const void *x" in header
    from whvi_amd import _hip
    L = _hip.lib()
    for name in ("whvi_diag_apply_stacked_bwd_f32", "whvi_diag_apply_stacked_bwd_supported", "whvi_diag_apply_stacked_bwd_slabs"):
        assert hasattr(L, name), name
    assert callable(_hip.diag_apply_stacked_bwd) and callable(_hip.diag_apply_stacked_bwd_supported)


def test_argument_checks_without_gpu():
    from whvi_amd import _hip
    L = _hip.lib()
    buf = (ctypes.c_char * (1 << 17))()
    p = (ctypes.addressof(buf) + 15) & ~15
    gx, out, part, g, x, s1, s2, u, bias = (p + 8192 * i for i in range(9))
    f = L.whvi_diag_apply_stacked_bwd_f32

    def call(gx=gx, out=out, part=part, g=g, x=x, s1=s1, s2=s2, u=u, bias=None, S=2, B=3, log2d=4, J=2, n_cols=20, ld_g=24,
             n_slabs=1, flags=2):
        return f(gx, out, part, g, x, s1, s2, u, bias, S, B, log2d, J, n_cols, ld_g, n_slabs, flags, None)

    # (none of these launches: a launch on this host would answer WHVI_ERR_LAUNCH = -4, which no check below accepts)
    for bad in (dict(S=-1), dict(B=-1), dict(J=-1), dict(n_cols=-1), dict(ld_g=-1), dict(n_slabs=-1)):
        assert call(**bad) == ERR_ARG and "negative" in _hip.last_error(), bad
    assert call(flags=64) == ERR_ARG and "unknown flags" in _hip.last_error()
    assert call(flags=256) == ERR_ARG and "unknown flags" in _hip.last_error()
    assert call(log2d=1) == ERR_SIZE and "log2(D)" in _hip.last_error()
    assert call(log2d=13) == ERR_SIZE and "log2(D)" in _hip.last_error()
    assert call(J=0) == ERR_SIZE and "n_blocks" in _hip.last_error()
    assert call(J=513, n_cols=1, ld_g=1) == ERR_SIZE and "8192" in _hip.last_error()           # 513 * 16 > 8192
    assert call(log2d=12, J=3, n_cols=1, ld_g=1) == ERR_SIZE and "8192" in _hip.last_error()
    assert call(n_cols=0) == ERR_ARG and "n_cols" in _hip.last_error()
    assert call(n_cols=33, ld_g=40) == ERR_ARG and "n_cols" in _hip.last_error()               # J D = 32
    assert call(n_cols=20, ld_g=19) == ERR_ARG and "ld_g" in _hip.last_error()
    assert call(S=0) == 0 and _hip.last_error() == ""                                          # nothing to do: no launch
    assert call(B=0, out=None, x=None, g=None, part=None) == 0 and _hip.last_error() == ""
    assert call(S=1 << 16, B=1 << 16) == ERR_SIZE and "32 bits" in _hip.last_error()
    assert call(S=1 << 40, B=1 << 40) == ERR_SIZE and "32 bits" in _hip.last_error()           # (the product overflows 64 bits)
    for name in ("out", "part", "g", "x", "s1", "s2", "u"):
        assert call(**{name: None}) == ERR_ARG and "null pointer" in _hip.last_error(), name
    for name in ("gx", "out", "part", "x", "s1", "s2", "u", "bias"):
        assert call(**{name: locals()[name] + 4}) == ERR_ALIGN and "aligned" in _hip.last_error(), name
    assert call(g=g + 2) == ERR_ALIGN and "aligned" in _hip.last_error()
    # a slab count must be one that ceil(B / ceil(B / n)) gives back: B = 5 has 1, 2, 3 and 5
    assert call(n_slabs=0) == ERR_ARG and "slab" in _hip.last_error()
    assert call(n_slabs=4) == ERR_ARG and "slab" in _hip.last_error()                          # more slabs than rows
    assert call(B=5, n_slabs=4) == ERR_ARG and "not a slab count" in _hip.last_error()
    assert call(S=65536, B=1, u=None) == ERR_ARG                                               # (checks run in order: the null pointer first)
    assert call(S=65536, B=1) == ERR_SIZE and "65535 samples" in _hip.last_error()             # the finishing launch's grid
    # grad_x: S B D = 96 floats = 384 bytes; out: 4 J U D = 4 * 2 * 3 * 16 floats = 1536 bytes; part: S * 1 * 2 * 20 floats = 320 bytes (the written columns)
    # g: 5 rows at pitch 24 + 20 columns = 140 floats = 560 bytes
    assert call(gx=x) == ERR_OVERLAP and "overlaps" in _hip.last_error()
    assert call(gx=g + 544) == ERR_OVERLAP and call(gx=g - 368) == ERR_OVERLAP
    assert call(out=g) == ERR_OVERLAP and call(out=x - 1520) == ERR_OVERLAP
    assert call(out=u + 16) == ERR_OVERLAP and call(out=s1 + 112) == ERR_OVERLAP and call(out=s2 - 16) == ERR_OVERLAP
    assert call(part=x + 368) == ERR_OVERLAP                                                   # a per-sample x: S B D = 384 bytes
    assert call(part=x + 176, flags=2 | 1) == ERR_OVERLAP                                      # a shared one: B D = 192 bytes
    assert call(part=bias - 304, bias=bias, flags=2 | 8) == ERR_OVERLAP                        # bias: J D = 128 bytes
    assert call(part=g - 304) == ERR_OVERLAP
    # a NULL grad_x is neither a null-pointer nor an alignment error: the call gets as far as the checks behind those
    assert call(gx=None, n_slabs=4) == ERR_ARG and "slab" in _hip.last_error()
    assert call(gx=None, out=g) == ERR_OVERLAP


def test_both_supported_rules_agree():
    from whvi_amd import _hip
    L = _hip.lib()
    for log2d in range(0, 14):
        for J in range(1, 601):
            want = bool(L.whvi_diag_apply_stacked_bwd_supported(log2d, J))
            assert _hip.diag_apply_stacked_bwd_supported(torch.float32, 1 << log2d, J) == want, (log2d, J)
            # (no instantiation needs scratch: the backward covers what the forward covers)
            assert want == bool(L.whvi_diag_apply_stacked_supported(log2d, J)), (log2d, J)
    assert not L.whvi_diag_apply_stacked_bwd_supported(4, 0) and not _hip.diag_apply_stacked_bwd_supported(torch.float32, 16, 0)
    assert not _hip.diag_apply_stacked_bwd_supported(torch.float64, 16, 1)
    assert _hip.diag_apply_stacked_bwd_supported(torch.float32, 4096, 2) and not _hip.diag_apply_stacked_bwd_supported(torch.float32, 4096, 3)


def test_slab_count_is_deterministic_and_at_least_one():
    from whvi_amd import _hip
    f = _hip.lib().whvi_diag_apply_stacked_bwd_slabs
    for S, B, log2d, J, n_cols in ((1, 1, 2, 1, 2), (3, 37, 10, 1, 2), (4, 512, 10, 1, 2), (8, 1000, 7, 4, 512), (3, 259, 4, 16, 253),
                                   (0, 0, 4, 1, 1), (3, 37, 20, 1, 1), (1, 1 << 30, 12, 2, 8192)):
        n = f(S, B, log2d, J, n_cols)
        assert n >= 1 and n == f(S, B, log2d, J, n_cols), (S, B, log2d, J, n_cols)
        if B >= 1:
            assert n <= B and -(-B // -(-B // n)) == n          # a slab count the launch accepts
    assert f(3, 37, 10, 1, 2) == f(3, 37, 10, 1, 1024)           # the narrowing does not change the geometry


def _layer(n_in, n_out, bias=True, flag=False, backward=False, seed=3):
    from whvi_amd.weights import WHVIStackedMatrix
    torch.manual_seed(seed)
    layer = WHVIStackedMatrix(n_in, n_out, bias=bias)
    layer.diag_blocks, layer.diag_blocks_backward = flag, backward
    return layer


def _net(n_in, flag, backward):
    from whvi_amd.layers import WHVILinear
    from whvi_amd.networks import WHVIRegression
    torch.manual_seed(5)
    net = WHVIRegression([WHVILinear(n_in, 128, bias=True), nn.ReLU(), WHVILinear(128, 128, bias=True), nn.ReLU(),
                          WHVILinear(128, 2, bias=True)], train_samples=3)
    return net.set_stacked_diagonal(flag, backward=backward)


def test_flag_is_a_class_default_and_the_network_sets_both():
    from whvi_amd.weights import WHVIStackedMatrix
    assert WHVIStackedMatrix.diag_blocks_backward is False
    net = _net(16, False, False)
    stacked = [m for m in net.modules() if isinstance(m, WHVIStackedMatrix)]
    assert len(stacked) == 2 and not any(m.diag_blocks or m.diag_blocks_backward for m in stacked)
    assert net.set_stacked_diagonal() is net and all(m.diag_blocks and not m.diag_blocks_backward for m in stacked)
    assert net.set_stacked_diagonal(True, True) is net and all(m.diag_blocks and m.diag_blocks_backward for m in stacked)
    net.set_stacked_diagonal(True)                               # callable as before: the backward goes back to its default
    assert all(m.diag_blocks and not m.diag_blocks_backward for m in stacked)
    net.set_stacked_diagonal(on=False, backward=True)            # no backward flag without the route
    assert not any(m.diag_blocks or m.diag_blocks_backward for m in stacked)


def test_flag_changes_nothing_on_host_tensors():
    x = torch.randn(9, 16)
    outs = []
    for flag in (False, True):
        layer = _layer(16, 130, flag=flag, backward=flag)
        torch.manual_seed(11)
        one = layer(x)
        mc = layer.forward_mc(x, 3, relu_in=True, relu_out=True)
        mc3 = layer.forward_mc(torch.randn(3, 9, 16), 3)
        outs.append((one, mc, mc3, layer.kl))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    losses = []
    for flag in (False, True):
        net = _net(8, flag, flag)
        torch.manual_seed(13)
        xb, yb = torch.randn(7, 8), torch.randn(7, 2)
        loss = net.loss(xb, yb, n=100)
        loss.backward()
        losses.append((loss.detach(), [p.grad.clone() for p in net.parameters()]))
    assert torch.equal(losses[0][0], losses[1][0])
    assert all(torch.equal(a, b) for a, b in zip(losses[0][1], losses[1][1]))


def test_copies_and_pickles_keep_the_flag_and_the_state_dict_keys_do_not_change():
    plain, flagged = _layer(16, 130), _layer(16, 130, flag=True, backward=True)
    assert list(plain.state_dict().keys()) == list(flagged.state_dict().keys())
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), flagged.state_dict().values()))
    for clone in (copy.deepcopy(flagged), pickle.loads(pickle.dumps(flagged))):
        assert clone.diag_blocks_backward is True and list(clone.state_dict().keys()) == list(plain.state_dict().keys())
    assert copy.deepcopy(plain).diag_blocks_backward is False
    from whvi_amd.weights import WHVIStackedMatrix
    fresh = WHVIStackedMatrix(16, 130, bias=True)
    assert "diag_blocks_backward" not in fresh.__dict__          # the default stays the class's: pickles from before load with it
    old = fresh.__reduce_ex__(2)[2]
    assert "diag_blocks_backward" not in old and pickle.loads(pickle.dumps(fresh)).diag_blocks_backward is False
    packed = _layer(16, 130, flag=True, backward=True).pack_parameters()
    assert list(packed.state_dict().keys()) == list(plain.state_dict().keys())
    clone = pickle.loads(pickle.dumps(packed))
    assert clone.diag_blocks_backward is True and clone._packed
    net = _net(16, True, True)
    assert list(net.state_dict().keys()) == list(_net(16, False, False).state_dict().keys())
    assert all(m.diag_blocks_backward for m in copy.deepcopy(net).modules() if hasattr(type(m), "diag_blocks_backward"))


def test_flag_on_create_graph_ops_match_float64_autograd_of_the_expression():
    """With ``native_backward`` the Function keeps (x, s1, s2, u, bias) and, where a graph is recorded, runs the torch ops with
    the output activation's mask recomputed from them: checked on the host against float64 autograd of ``_reference_ops`` at
    the existing host test's four (n_cols, shared, mean_plus) combinations, and that the result is differentiable."""
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
        ctx.bias_shape, ctx.needs_input_grad, ctx.native_backward = (1, J * D), (True,) * 5, True
        leaves = [t.clone().requires_grad_() for t in (x, s1, s2, u)]
        ctx.saved_tensors = (*leaves, bias)
        with torch.enable_grad():
            got = F_.backward(ctx, go.clone().requires_grad_())
        assert len(got) == 11 and all(t is None for t in got[5:])
        for a, b in zip(got[:5], want):
            assert a.shape == b.shape
            assert float((a.detach().double() - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-30, (n_cols, shared)
        assert all(t.requires_grad for t in got[:4])             # first-order gradients that can be differentiated again
        torch.autograd.grad(sum((t * t).sum() for t in got[:4]), leaves)


def test_flag_off_keeps_the_saved_tensor_layout():
    """A bare stand-in ctx without the new attribute takes the torch ops on (x, s1, s2, u, out), as before."""
    from whvi_amd.weights import StackedDiagApplyFunction as F_

    class Ctx:
        pass

    g = torch.Generator().manual_seed(3)
    J, D, S, B, n_cols = 2, 8, 2, 4, 13
    x, s1, s2 = torch.randn(S, B, D, generator=g), torch.randn(J, D, generator=g), torch.randn(J, D, generator=g)
    u, bias, go = torch.randn(J, S + 1, D, generator=g), torch.randn(J * D, generator=g), torch.randn(S, B, n_cols, generator=g)
    out = F_._reference_ops(x, s1, s2, u, bias, n_cols, True, False, True)
    res = []
    for flag in (None, False, True):
        ctx = Ctx()
        ctx.n_samples, ctx.n_cols, ctx.mean_plus, ctx.relu_in, ctx.relu_out = S, n_cols, True, False, True
        ctx.bias_shape, ctx.needs_input_grad = (J * D,), (True,) * 5
        if flag is not None:
            ctx.native_backward = flag
        ctx.saved_tensors = (x, s1, s2, u, bias if flag else out)
        with torch.enable_grad():
            res.append(F_.backward(ctx, go)[:5])
    for a, b, c in zip(*res):
        assert torch.equal(a, b) and torch.equal(a, c)           # (finite data: the recomputed mask is the saved output's)


def test_case_table_meets_every_switch_at_every_row_length():
    import stacked_diag_bwd_cases as bc
    from whvi_amd import _hip
    assert set(bc.DIMS) == {4, 16, 64, 128, 256, 512, 1024, 2048, 4096}
    for D in bc.DIMS:
        cases = [c for c in bc.CASES if c.D == D and not c.tune]
        for field in ("S", "shared", "bias", "relu_in", "relu_out", "mean_plus", "need_gx"):
            assert len({getattr(c, field) for c in cases}) == 2, (D, field)
        assert {c.B for c in cases} >= ({1, 37, 259} if D <= 256 else {1, 37})
        geoms = {(c.J, c.n_cols, c.ld_out) for c in cases}
        assert {(1, 2, 2), (1, 2, 8), (1, D, D)} <= geoms and len(geoms) >= 6
        assert any(ld == n and n % 4 for _, n, ld in geoms) and any(ld > n and J > 1 for J, n, ld in geoms)
    assert {(c.D, c.J) for c in bc.CASES} >= {(4, 64), (16, 16), (16, 64)}
    symbols = {bc.kernel_symbol(c) for c in bc.CASES}
    assert symbols == {f"whvi::stacked_diag_bwd_kernel<float, {c}, {nt}, {gx}>" for c in (1, 2, 4, 8)
                       for nt, gx in (("false", "false"), ("false", "true"), ("true", "true"))}
    # the exchange of products through LDS (more than one written block, grad_x wanted) and the direct store, per chunk count
    for cpt in (1, 2, 4, 8):
        assert {c.need_gx and c.n_cols > c.D for c in bc.CASES if bc.chunks_per_thread(c) == cpt} == {False, True}, cpt
    for c in bc.CASES + (bc.STREAM_CASE,):
        assert _hip.diag_apply_stacked_bwd_supported(torch.float32, c.D, c.J) and 1 <= c.n_cols <= c.J * c.D and c.ld_out >= c.n_cols
    assert len({bc.case_id(c) for c in bc.CASES}) == len(bc.CASES)
    s = bc.STREAM_CASE
    assert 4 * s.S * s.B * s.D > 256 << 20 and 4 * s.S * (s.B - 100) * s.D <= 256 << 20      # just over the threshold
    assert bc.kernel_symbol(s) == "whvi::stacked_diag_bwd_kernel<float, 1, true, true>"


def test_shipped_library_holds_the_kernels_without_scratch():
    from shipped_isa import ShippedLibrary
    with ShippedLibrary() as lib:
        found = {n for n in lib.kernels if n.startswith("whvi::stacked_diag_bwd_kernel<")}
        for c in (1, 2, 4, 8):
            for nt, gx in (("false", "false"), ("false", "true"), ("true", "true")):
                k = lib.find(f"whvi::stacked_diag_bwd_kernel<float, {c}, {nt}, {gx}>")
                assert k["scratch"] == 0 and k["lds"] == 0, (c, nt, gx, k)          # (the exchange tile is dynamic LDS)
                assert k["vgprs"] + k["agprs"] <= 512, (c, nt, gx, k["vgprs"], k["agprs"])
        assert len(found) == 12
        k = lib.find("whvi::stacked_diag_bwd_finish_kernel<float>")
        assert k["scratch"] == 0 and k["lds"] == 0
        # the forward's family keeps its own prefix: no backward kernel under it
        assert len([n for n in lib.kernels if n.startswith("whvi::diag_apply_stacked_kernel<")]) == 10
