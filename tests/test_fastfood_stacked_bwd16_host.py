"""The one-launch backward of the rectangular fastfood layer on 16-bit activations (whvi_fused_shs_stacked_bwd_f16 / _bf16,
``FastfoodStackedFunction(..., keep_half=True, fused_backward=True, fused_backward16=True)``) as far as it can be checked without
a GPU: the ABI declares and exports the three symbols, the support rule and its Python mirror, every refusal (ctypes with fake
aligned pointers: the checks happen before any device call; the extents of grad_x, grad_y and x are counted in 2-byte elements),
what the shipped library contains -- the 64 ``fused_stacked_bwd16_kernel<__half | __hip_bfloat16, L, K, J, nt>`` instantiations,
none with scratch, one new finishing kernel, and the unchanged pinned symbol sets -- that on host tensors the new flag changes
nothing, and the case list of tools/stacked_bwd16_table.py.

The overlap check at 2 bytes per element is decided here from the refusing side: a range that reaches into the last 16 bytes of
a 2-byte extent is refused, and the sizes are chosen so that ranges which only the 4-byte extents would reach lie apart.  The
accepting side needs a launch, so it is in tests/test_fastfood_stacked_bwd16_gpu.py (``grad_x`` directly behind ``x`` in one
buffer)."""
import ctypes
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ENTRIES = ("whvi_fused_shs_stacked_bwd16_supported", "whvi_fused_shs_stacked_bwd_f16", "whvi_fused_shs_stacked_bwd_bf16")
TYPES = ("__half", "__hip_bfloat16")
K16 = {6: 2, 7: 2, 8: 2, 9: 2, 10: 2, 11: 4}
SRC_SHARED = 4
ERR_ARG, ERR_SIZE, ERR_ALIGN, ERR_OVERLAP = -1, -2, -3, -5


def _rule(log2d, J):
    return (6 <= log2d <= 10 and 2 <= J <= 4) or (log2d == 11 and J == 2)


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
            assert L.whvi_fused_shs_stacked_bwd16_supported(log2d, J) == int(want), (log2d, J)
            for dtype in (torch.float16, torch.bfloat16):
                assert _hip.fused_shs_stacked_bwd16_supported(dtype, 1 << log2d, J) == want, (dtype, log2d, J)
            for dtype in (torch.float32, torch.float64):
                assert not _hip.fused_shs_stacked_bwd16_supported(dtype, 1 << log2d, J), (dtype, log2d, J)
    assert n_yes == 16                                     # times two dtypes and two cache policies: the 64 shipped kernels
    for log2d, J in ((-1, 2), (0, 2), (9, -1), (9, 1 << 40), (13, 2), (40, 2)):
        assert L.whvi_fused_shs_stacked_bwd16_supported(log2d, J) == 0, (log2d, J)
    assert not _hip.fused_shs_stacked_bwd16_supported(torch.float16, 100, 2)
    assert not _hip.fused_shs_stacked_bwd16_supported(torch.bfloat16, 0, 2)
    # the float32 query stays float32-only
    assert not _hip.fused_shs_stacked_bwd_supported(torch.float16, 256, 2)


def test_refusals_before_any_device_call():
    from whvi_amd import _hip
    buf = (ctypes.c_char * (1 << 20))()
    p = (ctypes.addressof(buf) + 15) & ~15
    K = 65536
    # J = 2, S = 2, stride = 2, D = 512: grad_y 8 KiB, x 4 KiB (2 shared), grad_x 4 KiB -- 2-byte elements; a / c 4 KiB, b 8 KiB,
    # grad_a / grad_c 4 KiB, grad_b 8 KiB -- float32; the workspace 2 blocks * 12 KiB
    names = ("grad_x", "grad_a", "grad_b", "grad_c", "work", "grad_y", "x", "a", "b", "c")
    ptrs = {name: p + (i + 1) * K for i, name in enumerate(names)}
    assert _hip.lib().whvi_fused_shs_stacked_bwd_workspace(2, 2, 9, 2) == 2 * 12288
    err = _hip.last_error
    for sfx in ("f16", "bf16"):
        fn = getattr(_hip.lib(), "whvi_fused_shs_stacked_bwd_" + sfx)

        def call(J=2, S=2, stride=2, log2d=9, flags=0, **over):
            args = dict(ptrs)
            args.update(over)
            return fn(*(args[n] for n in names), J, S, stride, log2d, flags, None)

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
        assert call(S=1 << 21, stride=1) == ERR_SIZE and "gradients are indexed with 32 bits" in err()
        assert call(J=4, S=1 << 20, stride=1) == ERR_SIZE and "gradients" in err()
        for name in names:
            assert call(**{name: ptrs[name] + 4}) == ERR_ALIGN and "aligned" in err(), name
            assert call(**{name: ptrs[name] + 2}) == ERR_ALIGN and "aligned" in err(), name
        # null before the limits before alignment before overlap
        assert call(a=None, x=ptrs["x"] + 4) == ERR_ARG and call(S=1 << 21, stride=1, x=ptrs["x"] + 4) == ERR_SIZE
        assert call(grad_x=ptrs["x"] + 4) == ERR_ALIGN
        # every output and the workspace over every input (first and last 16 bytes), the activations at 2 bytes an element
        size_in = {"grad_y": 8192, "x": 4096, "a": 4096, "b": 8192, "c": 4096}
        size_out = {"grad_x": 4096, "grad_a": 4096, "grad_b": 8192, "grad_c": 4096, "work": 24576}
        for o, ob in size_out.items():
            for i, ib in size_in.items():
                assert call(**{o: ptrs[i]}) == ERR_OVERLAP and "overlap" in err(), (o, i)
                assert call(**{o: ptrs[i] + ib - 16}) == ERR_OVERLAP, (o, i)
                assert call(**{o: ptrs[i] - ob + 16}) == ERR_OVERLAP, (o, i)
        assert call(grad_x=ptrs["x"] + 2048 - 16, flags=SRC_SHARED) == ERR_OVERLAP    # (a shared x is sample_stride rows: 2 KiB)
        assert call(grad_x=None, grad_a=ptrs["grad_y"] + 8192 - 16) == ERR_OVERLAP   # (J segments of grad_y are counted)
        assert call(grad_x=None, grad_a=ptrs["grad_y"] - 4096 + 16) == ERR_OVERLAP


def _shipped():
    import shipped_isa
    return shipped_isa.ShippedLibrary()


def test_shipped_library_has_the_64_instantiations_and_keeps_the_pinned_symbol_sets():
    import stacked_bwd16_table as tb
    with _shipped() as lib:
        kernels = lib.kernels
    mine = {n: k for n, k in kernels.items() if n.startswith("whvi::fused_stacked_bwd16_kernel<")}
    want = {f"whvi::fused_stacked_bwd16_kernel<{t}, {L}, {K16[L]}, {J}, {nt}>"
            for t in TYPES for L in range(6, 12) for J in range(2, 5) if _rule(L, J) for nt in ("true", "false")}
    assert len(want) == 64 and set(mine) == want
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgprs"] + k["agprs"] <= 512, (name, k)
    finish = [n for n in kernels if "stacked_bwd16" in n and n not in mine]
    assert finish == ["whvi::fused_stacked_bwd16_finish_kernel"], finish
    assert len([n for n in kernels if "fused_shs_stacked_bwd_finish_kernel" in n]) == 1
    # the case list reaches exactly the shipped symbols
    assert tb.reached() == set(mine) | set(finish)
    # the pinned sets, as tests/test_fastfood_stacked_bwd_host.py has them
    golden = [g for g in open(os.path.join(ROOT, "tests", "golden", "fused_shs_kernel_symbols_f32_f64.txt")).read().split("\n")
              if g.strip()]
    assert sorted(n for n in kernels if re.match(r"whvi::fused_shs_kernel<(float|double), ", n)) == sorted(golden)
    k_of = {"float": (4, 4, 4, 4, 4, 8, 16), "__half": (2, 2, 2, 2, 2, 4, 8), "__hip_bfloat16": (2, 2, 2, 2, 2, 4, 8)}
    bwd = {f"whvi::fused_shs_bwd_kernel<{t}, {L}, {ks[L - 6]}, {nt}>" for t, ks in k_of.items() for L in range(6, 13)
           for nt in ("true", "false")}
    assert {n for n in kernels if n.startswith("whvi::fused_shs_bwd_kernel<")} == bwd
    fwd = {f"whvi::fused_shs_stacked_kernel<float, {L}, {8 if L == 11 else 4}, {nt}>" for L in range(6, 12) for nt in ("true", "false")}
    assert {n for n in kernels if n.startswith("whvi::fused_shs_stacked_kernel<")} == fwd
    sbwd = {f"whvi::fused_shs_stacked_bwd_kernel<float, {L}, {8 if L == 11 else 4}, {J}, {nt}>"
            for L in range(6, 12) for J in range(2, 5) if _rule(L, J) for nt in ("true", "false")}
    assert {n for n in kernels if n.startswith("whvi::fused_shs_stacked_bwd_kernel<")} == sbwd


def test_case_list():
    import slab_table as st
    import stacked_bwd16_table as tb
    assert len(tb.CASES) == 64 and len({c["id"] for c in tb.CASES}) == 64
    seen = {}
    for c in tb.CASES:
        L, S, B = c["log2d"], c["S"], c["B"]
        la = tb.launch(c)
        assert S == 3 and _rule(L, c["J"]) and st.ragged(S, B, L), c
        assert la.tiles_per_wave == st.tiles_per_wave(S, B, L) and la.grid == S * st.fused_bwd_geom(S, B, L)[0]
        assert la.symbols == (la.symbol, "whvi::fused_stacked_bwd16_finish_kernel")
        if c["regime"] == "walk":
            assert not la.nt and la.tiles_per_wave >= 3 and tb.streamed_bytes(c) <= st.NT_MIN_BYTES, c
        else:
            assert la.nt and la.tiles_per_wave >= 2 and st.NT_MIN_BYTES < tb.streamed_bytes(c) < 1.5 * st.NT_MIN_BYTES, c
        seen.setdefault((c["dtype"], L, c["J"]), set()).add(c["regime"])
        for opt in ("shared", "need_x", "poison"):
            seen.setdefault((c["regime"], opt), set()).add(c[opt])
    for t in TYPES:
        for L, J in tb.SHIPPED_LJ:
            assert seen[(t, L, J)] == {"walk", "stream"}, (t, L, J)
    for regime in ("walk", "stream"):
        for opt in ("shared", "need_x", "poison"):
            assert seen[(regime, opt)] == {False, True}, (regime, opt)
    # the one-tile slices test (b) compares with are cached and one tile per wave
    for L, _ in tb.SHIPPED_LJ:
        per = st.one_tile_rows(L)
        sub = dict(dtype="__half", log2d=L, J=2, S=1, B=per, shared=False, need_x=True)
        assert tb.launch(sub).tiles_per_wave == 1 and not tb.launch(sub).nt, L


def test_the_flag_changes_nothing_on_host_tensors():
    from whvi_amd.fastfood import FastfoodStackedFunction, WHVIFastfoodStackedMatrix
    assert WHVIFastfoodStackedMatrix.fused_backward16 is False
    D, J, S, B = 16, 3, 2, 5
    g = torch.Generator().manual_seed(1)
    for shared in (False, True):
        x = torch.randn(B if shared else S * B, D, generator=g)
        a, c, b = torch.randn(J, D, generator=g), torch.randn(J, D, generator=g), torch.randn(J, S, D, generator=g)
        gy = torch.randn(S * B, J * D, generator=g)
        got = {}
        for flag in (False, True):
            leaves = [t.clone().requires_grad_() for t in (x, a, b, c)]
            y = FastfoodStackedFunction.apply(*leaves, S, B, shared, True, True, flag)
            y.backward(gy)
            got[flag] = [y.detach()] + [t.grad for t in leaves]
        for u, v in zip(got[False], got[True]):
            assert u is not None and torch.equal(u, v)
        # the nine-argument call keeps working
        leaves = [t.clone().requires_grad_() for t in (x, a, b, c)]
        FastfoodStackedFunction.apply(*leaves, S, B, shared, True, True).backward(gy)
        for u, v in zip(got[False][1:], (t.grad for t in leaves)):
            assert torch.equal(u, v)
