"""tools/stacked_diag_bwd_cases.py -- the case table of whvi_diag_apply_stacked_bwd_f32, shared by
tests/test_stacked_diag_bwd_gpu.py, tests/test_stacked_diag_bwd_host.py and tools/stacked_diag_bwd_rate.py: the launch's
shapes, its operands, the launch itself into sentinel-guarded buffers, the composition of existing launches its ``grad_x`` must
equal bit for bit, the float64 reference of its ``out`` and the error bound that follows from its summation tree.

A case is the forward table's ``Case`` (tools/stacked_diag_cases.py; its ``ld_out`` is the pitch of ``g`` here) with one more
switch, ``need_gx``.  ``CASES`` crosses D in {4, 16, 64, 128, 256, 512, 1024, 2048, 4096} with the forward's six geometries

    (1, 2, 2)  (1, 2, 8)  (1, D, D)  (J, (J - 1) D + min(5, D - 1), same)  (J, J D, J D + 4)  (J', J' D - 4, J' D)      J = 3, J' = 4

(J and J' lowered to J D <= 8192: 2 at D = 4096, 4 at D = 2048), S in {1, 3}, B in {1, 37, 259} (259 up to D = 256), and
deals shared / per-sample x, bias, each ReLU, mean_plus and need_gx so that every D meets both values of every switch and
every chunk count per thread (1, 2, 4, 8) meets both values of need_gx.  One more case per chunk count forces the non-temporal
stores, three give D = 4, 16 and 64 at least 256 / D blocks (a row of 64 .. 256 chunks: one row group, or a few), and
``STREAM_CASE`` is the one launch whose ``grad_x`` is large enough to stream by itself.  Operands are the forward table's with
``special=False``: finite, with the -0 and +0 in ``x`` that exercise the ``relu_in`` mask."""
import collections
import ctypes
import itertools

import torch

import stacked_diag_cases as sc

BwdCase = collections.namedtuple("BwdCase", sc.Case._fields + ("need_gx",))
DIMS = sc.DIMS
DIAG_TUNE_NT = sc.DIAG_TUNE_NT
SENTINEL = 12345.5
GUARD = 64                     # floats either side of grad_x, out and part
MAX_COLS = 8192                # J D of whvi_diag_apply_stacked_bwd_supported


def _geometries(D):
    most = MAX_COLS // D
    j3, j4, r = min(3, most), min(4, most), min(5, D - 1)
    return ((1, 2, 2), (1, 2, 8), (1, D, D), (j3, (j3 - 1) * D + r, (j3 - 1) * D + r), (j3, j3 * D, j3 * D + 4),
            (j4, j4 * D - 4, j4 * D))


def _cases():
    out = []
    for k, g in itertools.product(range(len(DIMS)), range(6)):      # the row length's number, the geometry's number
        D = DIMS[k]
        J, n_cols, ld = _geometries(D)[g]
        bits = (g * 11 + k * 8 + (g * k) % 5) & 31          # the forward table's five switches
        batches = (1, 37, 259) if D <= 256 else (1, 37, 37)
        out.append(BwdCase(D, J, n_cols, ld, (1, 3)[(g + k) % 2], batches[(g + 2 * k) % 3], bool(bits & 1), bool(bits & 2),
                           bool(bits & 4), bool(bits & 8), bool(bits & 16) or (g + k) % 4 != 0, 0, (g + k // 2) % 2 == 0))
    for D in (64, 512, 1024, 2048, 4096):                   # one forced non-temporal launch per chunk count (1, 2, 4, 8, 8)
        J = min(3, MAX_COLS // D)
        out.append(BwdCase(D, J, J * D - 3, J * D, 3, 5, D == 512, True, True, True, True, DIAG_TUNE_NT, True))
    # short rows with J >= 256 / D: the row is 64 .. 256 chunks wide
    out.append(BwdCase(4, 64, 253, 256, 3, 37, False, True, True, True, True, 0, True))
    out.append(BwdCase(16, 16, 253, 256, 1, 259, True, False, False, True, True, 0, True))
    out.append(BwdCase(16, 64, 1024, 1024, 3, 37, True, True, True, False, True, 0, False))
    return tuple(out)


CASES = _cases()
# just over 256 MiB of grad_x (4 * 16400 * 1024 * 4 bytes) for a WHVILinear(1024, 2) output layer: two columns of g
STREAM_CASE = BwdCase(1024, 1, 2, 2, 4, 16400, False, True, True, False, True, 0, True)


def case_id(c):
    return sc.case_id(c) + ("-gx" if c.need_gx else "")


# ---- the launch's geometry, restated (whvi_amd/csrc/diag_apply_stacked_bwd.hpp) -------------------------------------------
def chunks_per_thread(c):
    nc = c.J * c.D // 4
    return 1 if nc <= 256 else 2 if nc <= 512 else 4 if nc <= 1024 else 8


def row_groups(c):
    nc = c.J * c.D // 4
    return 256 // nc if nc < 256 else 1


def kernel_symbol(c):
    nt = "true" if (c.need_gx and (c.tune & DIAG_TUNE_NT or 4 * c.S * c.B * c.D > 256 << 20)) else "false"
    return f"whvi::stacked_diag_bwd_kernel<float, {chunks_per_thread(c)}, {nt}, {'true' if c.need_gx else 'false'}>"


def gamma(c, n_slabs):
    """Roundings on the longest path of one element of ``out``: a thread adds the rows of its slab that fall to its row group
    one after the other (ceil(slab_rows / RG) terms: as many additions, the first to an exact zero), the RG row groups are
    added in order (RG - 1), each of the finishing kernel's four accumulators takes ceil(n_slabs / 4) slabs and two more
    additions join them; every term is a rounded product (1) and the chain from the sum to the slot is at most four
    roundings (u0 * c, uk * c, their sum, the product with the sum -- slot 1)."""
    slab_rows = -(-c.B // n_slabs)
    rg = row_groups(c)
    return -(-slab_rows // rg) + (rg - 1) + -(-n_slabs // 4) + 2 + 1 + 4


def operands(c, device, seed=0):
    """(g (S B, ld) with NaN in the columns beyond n_cols, x, s1, s2, u, bias): finite operands, +-0 in x."""
    x, s1, s2, u, bias = sc.operands(c, device, special=False, seed=seed)
    gen = torch.Generator().manual_seed(77 + c.D + c.J + seed)
    g = torch.full((c.S, c.B, c.ld_out), float("nan"))
    g[..., :c.n_cols] = torch.randn(c.S, c.B, c.n_cols, generator=gen)
    return g.to(device), x, s1, s2, u, bias


def flags_of(c):
    return (1 if c.shared else 0) | (2 if c.mean_plus else 0) | (4 if c.relu_in else 0) | (8 if c.relu_out else 0) | c.tune


def launch(c, g, x, s1, s2, u, bias):
    """One call through the C ABI into sentinel-guarded buffers: (grad_x (S, B, D) view or None, out (4, J, U, D) view,
    the guarded buffers [(buffer, used elements)], n_slabs)."""
    from whvi_amd import _hip
    L = _hip.lib()
    dev = x.device
    U = c.S + (1 if c.mean_plus else 0)
    log2d = c.D.bit_length() - 1
    with torch.cuda.device(dev):
        n_slabs = int(L.whvi_diag_apply_stacked_bwd_slabs(c.S, c.B, log2d, c.J, c.n_cols))
        sizes = (c.S * c.B * c.D if c.need_gx else 0, 4 * c.J * U * c.D, c.S * n_slabs * 2 * (-(-c.n_cols // 4) * 4))
        bufs = [torch.full((n + 2 * GUARD,), SENTINEL, device=dev) for n in sizes]
        ptr = [b.data_ptr() + 4 * GUARD for b in bufs]
        rc = L.whvi_diag_apply_stacked_bwd_f32(ptr[0] if c.need_gx else None, ptr[1], ptr[2], g.data_ptr(), x.data_ptr(),
                                               s1.data_ptr(), s2.data_ptr(), u.data_ptr(), None if bias is None else bias.data_ptr(),
                                               c.S, c.B, log2d, c.J, c.n_cols, c.ld_out, n_slabs, flags_of(c),
                                               ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"whvi_diag_apply_stacked_bwd_f32: {rc}: {_hip.last_error()}")
    gx = bufs[0][GUARD:GUARD + sizes[0]].view(c.S, c.B, c.D) if c.need_gx else None
    out = bufs[1][GUARD:GUARD + sizes[1]].view(4, c.J, U, c.D)
    return gx, out, list(zip(bufs, sizes)), n_slabs


def guards_untouched(guarded):
    return all(bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + n:] == SENTINEL).all()) for b, n in guarded)


def composed_grad_x(c, g, x, s1, s2, u, bias):
    """What ``grad_x`` must equal bit for bit: ``_hip.diag_apply_bwd`` per written block on that block's columns of g (zero-extended
    for a ragged block) -- ``g_j * w_j`` with both masks -- added in ascending j with float32 torch adds."""
    from whvi_amd import _hip
    total = None
    for j in range(-(-c.n_cols // c.D)):
        n = min(c.D, c.n_cols - j * c.D)
        gj = torch.zeros(c.S, c.B, c.D, device=g.device)
        gj[..., :n] = g[..., j * c.D:j * c.D + n]
        part, _ = _hip.diag_apply_bwd(gj, x, s1[j], s2[j], u[j], n_samples=c.S, mean_plus=c.mean_plus, need_grad_x=True,
                                      bias=None if bias is None else bias[j * c.D:(j + 1) * c.D], relu_in=c.relu_in,
                                      relu_out=c.relu_out)
        total = part if total is None else total + part
    return total


def reference_out(c, g, x, s1, s2, u, bias):
    """(ref, terms): ``out`` (4, J, U, D) in float64 on the float32 forward's own mask, and the sum of the absolute terms of
    each element's sum (the scale of its rounding error).  Row 0 of a mean_plus ``out`` is the caller's: left at zero."""
    from whvi_amd import _hip
    J, D, S, n = c.J, c.D, c.S, c.n_cols
    gm = torch.zeros(S, c.B, J * D, dtype=torch.float64, device=g.device)
    gm[..., :n] = g[..., :n].double()
    if c.relu_out:
        fwd = _hip.diag_apply_stacked(x, s1, s2, u, bias, n_samples=S, n_cols=n, mean_plus=c.mean_plus, relu_in=c.relu_in,
                                      relu_out=True)
        gm[..., :n] *= (fwd > 0).double()
    xa = (torch.relu(x) if c.relu_in else x).double()
    x3 = (xa if xa.dim() == 3 else xa.unsqueeze(0)).unsqueeze(2)                       # (S or 1, B, 1, D)
    g4 = gm.view(S, c.B, J, D)
    gw, aw = (g4 * x3).sum(dim=1).transpose(0, 1), (g4 * x3).abs().sum(dim=1).transpose(0, 1)      # (J, S, D)
    gb, ab = g4.sum(dim=1).transpose(0, 1), g4.abs().sum(dim=1).transpose(0, 1)
    a, cc, ud, Dd = s1.double().unsqueeze(1), s2.double().unsqueeze(1), u.double(), float(D)
    m = 1 if c.mean_plus else 0
    uk, u0 = ud[:, m:], (ud[:, :1] if c.mean_plus else torch.zeros_like(ud[:, :1]))
    U = S + m
    ref = torch.zeros(4, J, U, D, dtype=torch.float64, device=g.device)
    terms = torch.zeros_like(ref)
    f = (a * Dd * cc, Dd * (u0 * cc) + Dd * (uk * cc), a * Dd * (u0 + uk))
    fa = ((a * Dd * cc).abs(), (Dd * u0 * cc).abs() + (Dd * uk * cc).abs(), (a * Dd).abs() * (u0.abs() + uk.abs()))
    for slot in range(3):
        ref[slot, :, m:], terms[slot, :, m:] = gw * f[slot], aw * fa[slot]
    ref[3, :, m:], terms[3, :, m:] = gb, ab
    return ref, terms
