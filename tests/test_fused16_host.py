"""The 16-bit fused pipeline (whvi_fused_shs_ex_f16 / _bf16) as far as it can be checked without a GPU: the ABI
declares and exports both entries, the Python boundary's support tables, the argument checks and refusals (ctypes with
fake aligned pointers: every check happens before any launch), and what the shipped library contains -- every
(dtype, log2d) instantiation, none with scratch, and every fused_shs_kernel<float|double, ...> symbol the library had
before the 16-bit kernels were added (tests/golden/fused_shs_kernel_symbols_f32_f64.txt)."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("whvi_fused_shs_ex_f16", "whvi_fused_shs_ex_bf16")
A_PER_SAMPLE, C_PER_SAMPLE, SRC_SHARED, ONE_TRANSFORM = 1, 2, 4, 8


def test_header_declares_and_library_exports_both_entries():
    from whvi_amd import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "whvi_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(whvi_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert "#define WHVI_HIP_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "whvi_hip.h")).read()
    assert _hip.lib().whvi_hip_abi_version() == 1


def test_support_tables():
    from whvi_amd import _hip
    want = {                       # dtype -> fused_supported at D = 4, 8, 8192, 16384
        torch.float32: (True, True, True, False),
        torch.float64: (True, True, False, False),
        torch.float16: (False, True, True, False),
        torch.bfloat16: (False, True, True, False),
        torch.int32: (False, False, False, False),
    }
    shared = {                     # fused_src_shared_supported: rows of >= 1 KiB, float32 / float64 only
        torch.float32: (False, False, True, False),
        torch.float64: (False, False, False, False),
        torch.float16: (False, False, False, False),
        torch.bfloat16: (False, False, False, False),
        torch.int32: (False, False, False, False),
    }
    for dtype in want:
        assert tuple(_hip.fused_supported(dtype, d) for d in (4, 8, 8192, 16384)) == want[dtype], dtype
        assert tuple(_hip.fused_src_shared_supported(dtype, d) for d in (4, 8, 8192, 16384)) == shared[dtype], dtype
    for dtype in (torch.float16, torch.bfloat16):
        assert all(_hip.fused_supported(dtype, 1 << k) for k in range(3, 14))
        assert not any(_hip.fused_src_shared_supported(dtype, 1 << k) for k in range(0, 15))
    assert _hip.fused_src_shared_supported(torch.float64, 128) and _hip.fused_src_shared_supported(torch.float32, 256)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_checks_and_refusals(entry):
    from whvi_amd import _hip
    fused = getattr(_hip.lib(), entry)
    buf = (ctypes.c_char * 65536)()
    p = (ctypes.addressof(buf) + 15) & ~15
    q, v = p + 16384, p + 32768                    # a second data buffer and a float32 vector, all disjoint
    COL, ROW = 1, 0

    def call(dst, src, a=None, b=None, c=None, rows=4, log2d=9, n_samples=2, stride=2, group_rows=1, axis=COL, flags=0):
        return fused(dst, src, a, b, c, rows, log2d, n_samples, stride, group_rows, axis, flags, None)

    def err():
        return _hip.last_error()

    # the f32 entry's list
    assert call(None, p) == -1 and "null" in err()
    assert call(p + 4, q) == -3 and "aligned" in err()
    assert call(q, p + 2) == -3 and "aligned" in err()
    assert call(q, p, a=v + 4) == -3 and "scale vectors" in err()
    assert call(q, p, b=v + 8) == -3 and call(q, p, c=v + 12) == -3
    assert call(p, p + 16) == -5 and "overlap" in err()                       # dst / src partial overlap
    assert call(q, p, rows=-1) == -1 and "negative" in err()
    assert call(q, p, n_samples=0) == -1 and call(q, p, stride=0) == -1 and call(q, p, group_rows=0) == -1
    assert call(p, p, rows=1 << 32, log2d=3) == -2 and "32 bits" in err()     # rows beyond the 32-bit row index
    assert call(q, p, n_samples=1 << 32) == -2
    assert call(q, p, log2d=14) == -2 and "supported range" in err()
    assert call(q, p, log2d=2) == -2 and "supported range" in err()
    assert call(q, p, log2d=-1) == -2
    assert call(q, p, axis=7) == -1 and "axis" in err()
    assert call(q, p, flags=16) == -1 and "unknown fused flags" in err()
    # dst must not overlap a scale vector (rows = 4, D = 512: dst is 4 KiB, a vector 2 KiB, b 4 KiB)
    assert call(q, p, a=q + 2048) == -5 and "scale vector" in err()
    assert call(q, p, b=q - 4096 + 16) == -5 and "scale vector" in err()
    assert call(q, p, c=q + 4096 - 16) == -5
    # the four refused forms, each named
    assert call(q, p, axis=ROW) == -1 and "row-axis" in err()
    assert call(q, None) == -1 and "identity-source" in err()
    assert call(q, p, flags=SRC_SHARED) == -1 and "shared-source" in err()
    assert call(q, p, flags=ONE_TRANSFORM) == -1 and "one-transform" in err()
    assert call(q, p, flags=SRC_SHARED | ONE_TRANSFORM | A_PER_SAMPLE) == -1
    # nothing to do: accepted without touching a pointer
    assert call(None, None, rows=0) == 0 and err() == ""
    assert call(q, p, rows=0, flags=A_PER_SAMPLE | C_PER_SAMPLE) == 0


def test_python_boundary_refuses_by_name_before_any_launch():
    """The refusals of _hip.fused_shs for 16-bit dtypes are decided on the arguments alone (``src=None`` needs no tensor)."""
    from whvi_amd import _hip
    for dtype in (torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError, match="src=None"):
            _hip.fused_shs(None, axis="col", rows=4, d=64, dtype=dtype, device="cpu")
        with pytest.raises(RuntimeError, match="axis='row'"):
            _hip.fused_shs(torch.zeros(4, 64, dtype=dtype), axis="row", group_rows=4)
        for form in ("src_shared", "one_transform"):
            with pytest.raises(RuntimeError, match=form):
                _hip.fused_shs(torch.zeros(4, 64, dtype=dtype), **{form: True})


def _shipped():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    return shipped_isa.ShippedLibrary()


def test_shipped_library_has_every_instantiation_without_scratch_and_keeps_the_f32_f64_symbols():
    with _shipped() as lib:
        kernels = lib.kernels
    for type_name in ("__half", "__hip_bfloat16"):
        for log2d in range(3, 14):
            mine = {n: k for n, k in kernels.items() if n.startswith(f"whvi::fused_shs16_kernel<{type_name}, {log2d}, ")}
            forms = {tuple(re.search(r"<(.*)>", n).group(1).split(", ")[3:6]) for n in mine}      # (NT, POLICY, STAGE)
            assert ("true", "0", "0") in forms and ("false", "0", "0") in forms, (type_name, log2d, sorted(forms))
            if log2d >= 9:             # rows of >= 64 chunks: a and c staged in LDS for launches that fill the chip
                assert ("true", "0", "1") in forms and ("false", "0", "1") in forms, (type_name, log2d, sorted(forms))
            for name, k in mine.items():
                assert k["scratch"] == 0 and k["agprs"] == 0, (name, k)
                k_chunks = int(re.search(r"<(.*)>", name).group(1).split(", ")[2])
                assert k_chunks == (16 if log2d == 13 else 8), name
                if 9 <= log2d <= 12:
                    assert k["vgprs"] <= 128, (name, k["vgprs"])        # four waves per SIMD
    golden = open(os.path.join(ROOT, "tests", "golden", "fused_shs_kernel_symbols_f32_f64.txt")).read().split("\n")
    golden = [g for g in golden if g.strip()]
    assert len(golden) > 50
    missing = [g for g in golden if g not in kernels]
    assert missing == [], missing[:5]
    now = sorted(n for n in kernels if re.match(r"whvi::fused_shs_kernel<(float|double), ", n))
    assert now == sorted(golden), "the float / double instantiations of fused_shs_kernel changed"
