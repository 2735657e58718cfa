"""The one-launch backward of the rectangular fastfood layer (whvi_fused_shs_stacked_bwd_f32,
``FastfoodStackedFunction(..., fused_backward=True)``) as far as it can be checked without a GPU: the ABI declares and exports the
three symbols, the support rule and its Python mirror, the workspace query against a restatement of ``fused_bwd_geom``, every
refusal (ctypes with fake aligned pointers: the checks happen before any device call), what the shipped library contains -- the 32
``fused_shs_stacked_bwd_kernel<float, L, K, J, nt>`` instantiations, none with scratch, and the unchanged sets of
``fused_shs_kernel`` / ``fused_shs_bwd_kernel`` / ``fused_shs_stacked_kernel`` symbols -- and, on host tensors, that the flag changes
nothing."""
import ctypes
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("whvi_fused_shs_stacked_bwd_supported", "whvi_fused_shs_stacked_bwd_workspace", "whvi_fused_shs_stacked_bwd_f32")
SRC_SHARED = 4
ERR_ARG, ERR_SIZE, ERR_ALIGN, ERR_OVERLAP = -1, -2, -3, -5


def _rule(log2d, J):
    return (6 <= log2d <= 10 and 2 <= J <= 4) or (log2d == 11 and J == 2)


def _n_slabs(S, stride, log2d):
    """``fused_bwd_geom(S, stride, log2d).n_slabs`` restated (whvi_amd/csrc/fused_bwd.hpp)."""
    rpt = max(1, 1024 >> log2d)
    n = min(-(-(512 if log2d >= 12 else 1024) // S), -(-stride // (4 * rpt)))
    n = max(n, 1)
    slab = -(-(-(-stride // n)) // rpt) * rpt
    return -(-stride // slab)


def test_header_declares_and_library_exports_the_three_symbols():
    from whvi_amd import _hip
    raw = open(os.path.join(ROOT, "include", "whvi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(whvi_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert "#define WHVI_HIP_ABI_VERSION 1" in raw
    assert _hip.lib().whvi_hip_abi_version() == 1


def test_support_rule_and_its_mirror():
    from whvi_amd import _hip
    L = _hip.lib()
    n_yes = 0
    for log2d in range(5, 13):
        for J in range(0, 7):
            want = _rule(log2d, J)
            n_yes += want
            assert L.whvi_fused_shs_stacked_bwd_supported(log2d, J) == int(want), (log2d, J)
            assert _hip.fused_shs_stacked_bwd_supported(torch.float32, 1 << log2d, J) == want, (log2d, J)
    assert n_yes == 16                                     # times the two cache policies: the 32 shipped kernels
    for log2d, J in ((-1, 2), (0, 2), (9, -1), (9, 1 << 40), (13, 2), (40, 2)):
        assert L.whvi_fused_shs_stacked_bwd_supported(log2d, J) == 0, (log2d, J)
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        assert not _hip.fused_shs_stacked_bwd_supported(dtype, 256, 2)
    assert not _hip.fused_shs_stacked_bwd_supported(torch.float32, 100, 2)
    assert not _hip.fused_shs_stacked_bwd_supported(torch.float32, 0, 2)


def test_workspace_query():
    from whvi_amd import _hip
    L = _hip.lib()
    q = L.whvi_fused_shs_stacked_bwd_workspace
    for S, stride, log2d, J in ((1, 1, 6, 2), (3, 5, 6, 4), (2, 777, 7, 3), (4, 64, 8, 2), (16, 8192, 10, 4), (64, 1000, 7, 4),
                                (16, 4096, 11, 2), (1, 256, 10, 4), (2000, 3, 9, 3), (8, 4096, 10, 4)):
        D = 1 << log2d
        n_slabs = _n_slabs(S, stride, log2d)
        assert q(S, stride, log2d, J) == S * n_slabs * 12 * D * J, (S, stride, log2d, J)
        # the grid is the per-block launch's: J of its slots per block
        assert q(S, stride, log2d, J) == J * L.whvi_fused_shs_bwd_workspace(S, stride, log2d), (S, stride, log2d, J)
    assert _n_slabs(16, 8192, 10) == 64 and _n_slabs(2, 777, 7) == 25 and _n_slabs(1, 1, 6) == 1
    for S, stride in ((0, 7), (7, 0), (0, 0)):
        assert q(S, stride, 9, 2) == 0
    assert q(-1, 4, 9, 2) == ERR_ARG and q(4, -1, 9, 2) == ERR_ARG and q(4, 4, 9, -1) == ERR_ARG
    for log2d, J in ((5, 2), (12, 2), (11, 3), (9, 0), (9, 1), (9, 5), (-1, 2)):
        assert q(4, 4, log2d, J) == ERR_SIZE, (log2d, J)
        assert q(0, 0, log2d, J) == ERR_SIZE, (log2d, J)


def test_refusals_before_any_device_call():
    from whvi_amd import _hip
    fn = _hip.lib().whvi_fused_shs_stacked_bwd_f32
    buf = (ctypes.c_char * (1 << 20))()
    p = (ctypes.addressof(buf) + 15) & ~15
    K = 65536
    # J = 2, S = 2, stride = 2, D = 512: grad_y 16 KiB, x 8 KiB (4 shared), a / c 4 KiB, b 8 KiB; grad_x 8 KiB, grad_a / grad_c
    # 4 KiB, grad_b 8 KiB, the workspace 2 blocks * 12 KiB
    names = ("grad_x", "grad_a", "grad_b", "grad_c", "work", "grad_y", "x", "a", "b", "c")
    ptrs = {name: p + i * K for i, name in enumerate(names)}
    assert _hip.lib().whvi_fused_shs_stacked_bwd_workspace(2, 2, 9, 2) == 2 * 12288

    def call(J=2, S=2, stride=2, log2d=9, flags=0, **over):
        args = dict(ptrs)
        args.update(over)
        return fn(*(args[n] for n in names), J, S, stride, log2d, flags, None)

    err = _hip.last_error
    for flags in (1, 2, 8, SRC_SHARED | 16):
        assert call(flags=flags) == ERR_ARG and "unknown fused flags" in err(), flags
    assert call(J=-1) == ERR_ARG and "negative" in err()
    assert call(S=-1) == ERR_ARG and call(stride=-1) == ERR_ARG
    for log2d in (-1, 0, 5, 12, 13):
        assert call(log2d=log2d) == ERR_SIZE and "supported range" in err(), log2d
    for J in (0, 1, 5, 6):
        assert call(J=J) == ERR_SIZE and "supported range" in err(), J
    assert call(log2d=11, J=3) == ERR_SIZE and call(log2d=11, J=4) == ERR_SIZE
    # flags before sizes before support before the empty call
    assert call(flags=1, J=-1) == ERR_ARG and "flags" in err()
    assert call(J=-1, log2d=3) == ERR_ARG and call(J=5, S=0) == ERR_SIZE
    # nothing to do: accepted without touching a pointer or a device
    assert call(S=0) == 0 and err() == ""
    assert call(stride=0) == 0 and err() == ""
    assert fn(*([None] * 10), 2, 0, 7, 9, 0, None) == 0
    assert fn(*([None] * 10), 4, 3, 0, 10, SRC_SHARED, None) == 0
    for name in names[1:]:
        assert call(**{name: None}) == ERR_ARG and "null" in err(), name
    assert call(S=1 << 20, stride=1 << 12) == ERR_SIZE and "rows are indexed with 32 bits" in err()
    assert call(S=1 << 21, stride=1) == ERR_SIZE and "gradients are indexed with 32 bits" in err()     # 2 * (2^21 + 2) * 512 >= 2^31
    assert call(J=4, S=1 << 20, stride=1) == ERR_SIZE and "gradients" in err()
    for name in names:
        assert call(**{name: ptrs[name] + 4}) == ERR_ALIGN and "aligned" in err(), name
    # null before the limits before alignment
    assert call(a=None, x=ptrs["x"] + 4) == ERR_ARG and call(S=1 << 21, stride=1, x=ptrs["x"] + 4) == ERR_SIZE
    # every output and the workspace over every input (first and last 16 bytes)
    size_in = {"grad_y": 16384, "x": 8192, "a": 4096, "b": 8192, "c": 4096}
    size_out = {"grad_x": 8192, "grad_a": 4096, "grad_b": 8192, "grad_c": 4096, "work": 24576}
    for o, ob in size_out.items():
        for i, ib in size_in.items():
            assert call(**{o: ptrs[i]}) == ERR_OVERLAP and "overlap" in err(), (o, i)
            assert call(**{o: ptrs[i] + ib - 16}) == ERR_OVERLAP, (o, i)
            assert call(**{o: ptrs[i] - ob + 16}) == ERR_OVERLAP, (o, i)
    assert call(grad_x=ptrs["x"] + 4096 - 16, flags=SRC_SHARED) == ERR_OVERLAP    # (a shared x is sample_stride rows: 4 KiB)
    assert call(grad_x=None, grad_a=ptrs["grad_y"] + 16384 - 16) == ERR_OVERLAP   # (J segments of grad_y are counted)


def _shipped():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    return shipped_isa.ShippedLibrary()


def test_shipped_library_has_the_32_instantiations_and_keeps_the_pinned_symbol_sets():
    with _shipped() as lib:
        kernels = lib.kernels
    mine = {n: k for n, k in kernels.items() if n.startswith("whvi::fused_shs_stacked_bwd_kernel<")}
    want = {f"whvi::fused_shs_stacked_bwd_kernel<float, {L}, {8 if L == 11 else 4}, {J}, {nt}>"
            for L in range(6, 12) for J in range(2, 5) if _rule(L, J) for nt in ("true", "false")}
    assert len(want) == 32 and set(mine) == want
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgprs"] + k["agprs"] <= 512, (name, k)
    assert len([n for n in kernels if "fused_shs_stacked_bwd_finish_kernel" in n]) == 1
    # the pinned sets, as tests/test_fastfood_stacked_host.py has them
    golden = [g for g in open(os.path.join(ROOT, "tests", "golden", "fused_shs_kernel_symbols_f32_f64.txt")).read().split("\n")
              if g.strip()]
    assert sorted(n for n in kernels if re.match(r"whvi::fused_shs_kernel<(float|double), ", n)) == sorted(golden)
    k_of = {"float": (4, 4, 4, 4, 4, 8, 16), "__half": (2, 2, 2, 2, 2, 4, 8), "__hip_bfloat16": (2, 2, 2, 2, 2, 4, 8)}
    bwd = {f"whvi::fused_shs_bwd_kernel<{t}, {L}, {ks[L - 6]}, {nt}>" for t, ks in k_of.items() for L in range(6, 13)
           for nt in ("true", "false")}
    assert {n for n in kernels if n.startswith("whvi::fused_shs_bwd_kernel<")} == bwd
    fwd = {f"whvi::fused_shs_stacked_kernel<float, {L}, {8 if L == 11 else 4}, {nt}>" for L in range(6, 12) for nt in ("true", "false")}
    assert {n for n in kernels if n.startswith("whvi::fused_shs_stacked_kernel<")} == fwd


def test_the_flag_changes_nothing_on_host_tensors():
    from whvi_amd.fastfood import FastfoodStackedFunction
    D, J, S, B = 16, 3, 2, 5
    g = torch.Generator().manual_seed(1)
    for shared in (False, True):
        x = torch.randn(B if shared else S * B, D, generator=g)
        a, c, b = torch.randn(J, D, generator=g), torch.randn(J, D, generator=g), torch.randn(J, S, D, generator=g)
        gy = torch.randn(S * B, J * D, generator=g)
        got = {}
        for flag in (False, True):
            leaves = [t.clone().requires_grad_() for t in (x, a, b, c)]
            y = FastfoodStackedFunction.apply(*leaves, S, B, shared, False, flag)
            y.backward(gy)
            got[flag] = [y.detach()] + [t.grad for t in leaves]
        for u, v in zip(got[False], got[True]):
            assert u is not None and torch.equal(u, v)
