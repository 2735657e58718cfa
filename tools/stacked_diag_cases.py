"""tools/stacked_diag_cases.py -- the case table of whvi_diag_apply_stacked_f32, shared by tests/test_stacked_diag_gpu.py and
tools/stacked_diag_rate.py: the launch's shapes, its operands (with the zeros, poisoned rows and non-finite parameters the
bit-for-bit check wants) and the composition of existing launches it must equal.

A case is ``Case(D, J, n_cols, ld_out, S, B, shared, bias, relu_in, relu_out, mean_plus, tune)``.  ``CASES`` crosses
D in {4, 16, 64, 128, 256, 512, 1024, 2048, 4096} -- both sides of the rows-per-wave switch (D = 256), every kernel
instantiation (chunks per lane 1, 2, 4, 8, 16) and the widest row -- with the output geometries

    (1, 2, 2)  (1, 2, 8)  (1, D, D)  (J, (J - 1) D + min(5, D - 1), same)  (J, J D, J D + 4)  (J', J' D - 4, J' D)      J = 3, J' = 4

(J and J' lowered to what 64 KiB of LDS holds: 2 at D = 4096, 4 at D = 2048), and deals S in {1, 3}, B in {1, 37, 259}
(259 up to D = 256: beyond, 37 rows are already several iterations per wave and several slabs), shared / per-sample x, bias,
each ReLU and mean_plus over them so that every D meets both values of every switch.  One more case per instantiation forces
the non-temporal stores (``DIAG_TUNE_NT``), three more give D = 4 and 16 as many blocks as a wave has lane groups (256 / D: from
there on the kernel's groups share their rows and split the blocks), and ``STREAM_CASE`` is the one launch large enough to
stream by itself."""
import collections
import itertools

import torch

Case = collections.namedtuple("Case", "D J n_cols ld_out S B shared bias relu_in relu_out mean_plus tune")

DIMS = (4, 16, 64, 128, 256, 512, 1024, 2048, 4096)
DIAG_TUNE_NT = 16


def _max_blocks(D):
    return 65536 // (8 * D)


def _geometries(D):
    j3, j4, r = min(3, _max_blocks(D)), min(4, _max_blocks(D)), min(5, D - 1)
    return ((1, 2, 2), (1, 2, 8), (1, D, D), (j3, (j3 - 1) * D + r, (j3 - 1) * D + r), (j3, j3 * D, j3 * D + 4),
            (j4, j4 * D - 4, j4 * D))


def _cases():
    out = []
    for k, g in itertools.product(range(len(DIMS)), range(6)):      # the row length's number, the geometry's number
        D = DIMS[k]
        J, n_cols, ld = _geometries(D)[g]
        bits = (g * 11 + k * 8 + (g * k) % 5) & 31          # five switches: every D meets 0 and 1 of each (checked on the host)
        batches = (1, 37, 259) if D <= 256 else (1, 37, 37)
        out.append(Case(D, J, n_cols, ld, (1, 3)[(g + k) % 2], batches[(g + 2 * k) % 3], bool(bits & 1), bool(bits & 2),
                        bool(bits & 4), bool(bits & 8), bool(bits & 16) or (g + k) % 4 != 0, 0))
    for D in (64, 512, 1024, 2048, 4096):                   # one forced non-temporal launch per instantiation
        J = min(3, _max_blocks(D))
        out.append(Case(D, J, J * D - 3, J * D, 3, 5, D == 512, True, True, True, True, DIAG_TUNE_NT))
    # short rows with at least as many blocks as lane groups per wave (256 / D): the groups share rows and split the blocks
    # (D = 64 with J = 4 and D = 128 are above; D = 64 with J = 3 and every J = 1 case take the other map)
    out.append(Case(4, 64, 253, 256, 3, 37, False, True, True, True, True, 0))
    out.append(Case(16, 16, 253, 256, 1, 259, True, False, False, True, True, 0))
    out.append(Case(16, 64, 1024, 1024, 3, 37, True, True, True, False, True, 0))
    return tuple(out)


CASES = _cases()
# just over 256 MiB written (4 * 4100 * 4096 * 4 bytes): the launch takes the non-temporal stores by its own rule
STREAM_CASE = Case(1024, 4, 4096, 4096, 4, 4100, False, True, False, True, True, 0)


def case_id(c):
    return (f"D{c.D}-J{c.J}-n{c.n_cols}-ld{c.ld_out}-S{c.S}-B{c.B}-{'sh' if c.shared else 'ps'}{'-b' if c.bias else ''}"
            f"{'-ri' if c.relu_in else ''}{'-ro' if c.relu_out else ''}{'-mp' if c.mean_plus else ''}{'-nt' if c.tune else ''}")


def operands(c, device, special=True, seed=0):
    """(x, s1, s2, u, bias) of a case on ``device``.  ``special``: -0 and +0 in x, one row with a single inf, one with a
    single NaN, one with two non-finite entries (batches of at least 4 rows), one ``s1[j, i] = inf`` and one ``u`` large
    enough to trip wbar_diag's half-sum rule; negative diagonals come with the signs of the draws either way."""
    g = torch.Generator().manual_seed(1000 * c.D + 10 * c.J + c.S + seed)
    U = c.S + (1 if c.mean_plus else 0)
    x = torch.randn((c.B, c.D) if c.shared else (c.S, c.B, c.D), generator=g)
    s1 = torch.randn(c.J, c.D, generator=g) * 0.3
    s2 = torch.randn(c.J, c.D, generator=g) * 0.3
    u = torch.randn(c.J, U, c.D, generator=g)
    bias = torch.randn(c.J * c.D, generator=g) if c.bias else None
    x3 = x if x.dim() == 3 else x.unsqueeze(0)
    x3[:, 0, 0], x3[:, 0, 1] = -0.0, 0.0
    if special:
        if c.B >= 4:
            x3[:, 1, 2 % c.D] = float("inf")
            x3[:, 2, 1] = float("nan")
            x3[:, 3, 0], x3[:, 3, c.D - 1] = float("-inf"), float("nan")
        s1[c.J - 1, 1] = float("inf")
        u[0, U - 1, 3 % c.D] = 3.0e38
        s2[0, 3 % c.D] = 1.0                               # v = u * s2 is finite, D / 2 * v is not: NaN by the half-sum rule
    return tuple(None if t is None else t.to(device) for t in (x, s1, s2, u, bias))


def composed(c, x, s1, s2, u, bias):
    """What the launch must equal bit for bit: ``_hip.diag_apply`` per block with that block's operands and bias slice, the
    blocks side by side, the first ``n_cols`` columns."""
    from whvi_amd import _hip
    parts = [_hip.diag_apply(x, s1[j], s2[j], u[j], None if bias is None else bias[j * c.D:(j + 1) * c.D], n_samples=c.S,
                             mean_plus=c.mean_plus, relu_in=c.relu_in, relu_out=c.relu_out) for j in range(c.J)]
    return torch.cat(parts, dim=2)[..., :c.n_cols]


def launch(c, x, s1, s2, u, bias, out=None):
    from whvi_amd import _hip
    return _hip.diag_apply_stacked(x, s1, s2, u, bias, n_samples=c.S, n_cols=c.n_cols, mean_plus=c.mean_plus,
                                   relu_in=c.relu_in, relu_out=c.relu_out, out=out, tune=c.tune)
