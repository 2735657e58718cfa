#!/usr/bin/env python3
"""tools/train_aux_ref.py -- host references for the small kernels every training step runs (whvi_amd/csrc/abi.hip:
whvi_reparam_kl_f32; whvi_amd/csrc/train_aux.hip: whvi_reparam_kl_philox_f32, whvi_reparam_kl_bwd_f32, whvi_gauss_mnll_f32,
whvi_gauss_mnll_bwd_f32), and the case list on which tests/test_train_aux_host.py and tests/test_train_aux_gpu.py hold them.

Three layers, numpy only (no torch, no GPU):

  * ``philox4x32_10`` and ``eps_reference``: the in-kernel draw restated on the host.  Philox4x32-10 (Salmon et al., SC'11)
    keyed by the 64-bit seed, one counter per (element column i, matrix j, block of eight samples z, call), Box-Muller on the
    four output words.  The counter layout below is the contract of include/whvi_hip.h; the uniforms and the angle repeat the
    kernel's float32 arithmetic exactly, the logarithm, square root, cosine and sine are float64.
  * ``reparam_kl_reference``, ``reparam_kl_bwd_reference``, ``gauss_mnll_reference``: the closed forms in float64 on the
    float32 inputs, each with its YARDSTICK -- the same expression with every term replaced by its absolute value.  A float32
    evaluation in any order errs by a small multiple of 2^-24 times the yardstick, per element, however the terms cancel; the
    tests bound |got - reference| by 1e-6 or 2e-6 of it (``BOUNDS``), element by element.
  * ``emulate_*``: the kernels' own float32 operation order in numpy (the 64-lane shuffle tree, the add of the four waves, the
    per-sample accumulation, the grid-stride loop of the MNLL reduction), with named mutations.  They exist so that the host
    test can show, without a GPU and without touching the shipped kernels, that the bounds are attainable (the emulation stays
    inside) and discriminating (each mutation leaves them on some case of the list).

    python tools/train_aux_ref.py        # the case list"""
import itertools
from collections import namedtuple

import numpy as np

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64

# ---- Philox4x32-10 ---------------------------------------------------------------------------------------------------------------
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85          # key increments (golden ratio, sqrt(3) - 1)
SAMPLES_PER_BLOCK = 8                                  # dispatch.hpp: REPARAM_SAMPLES_PER_BLOCK -- one blockIdx.z
CALLS_PER_BLOCK = SAMPLES_PER_BLOCK // 4               # the launch offset advances by this much
MASK32 = 0xFFFFFFFF

# Random123's known-answer vectors for philox4x32_10: (counter, key, result)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def _mulhilo(m, c):
    """High and low 32 bits of the 64-bit product of the constant m and the uint32 array c."""
    p = U64(m) * c.astype(U64)
    return (p >> U64(32)).astype(U32), (p & U64(MASK32)).astype(U32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox4x32 on uint32 arrays (broadcast against each other); returns the four output words."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(v, dtype=U32) for v in (c0, c1, c2, c3, k0, k1)))
    for _ in range(10):
        hi0, lo0 = _mulhilo(PHILOX_M0, c0)
        hi1, lo1 = _mulhilo(PHILOX_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = ((k0.astype(U64) + U64(PHILOX_W0)) & U64(MASK32)).astype(U32)
        k1 = ((k1.astype(U64) + U64(PHILOX_W1)) & U64(MASK32)).astype(U32)
    return c0, c1, c2, c3


def uniform24(x):
    """The kernel's map from a 32-bit word to a float32 uniform: the top 24 bits plus a half, times 2^-24, in float32.  The sum
    rounds once the 24-bit integer reaches 2^23 (ties to even), so the image is (0, 1]: 2^-25 at 0 and 1.0 at 2^24 - 1 only."""
    return (((np.asarray(x, dtype=U32) >> U32(8)).astype(F32) + F32(0.5)) * F32(2.0 ** -24)).astype(F32)


TWO_PI_F32 = F32(6.283185307179586)


def counters(offset, J, S, D, mutate=None):
    """The Philox counters of one launch: uint32 arrays (J, Z, C, D) for c0..c3 with Z = ceil(S / 8) sample blocks and C calls
    per block, sample k = 8 z + 4 call + (0..3).  ``mutate``: None -- the kernel's layout; "swap_words" -- counter words 0 and 1
    exchanged; "eight_call" -- the eight samples of a block drawn as eight calls (call = q), one normal of each used."""
    Z = (S + SAMPLES_PER_BLOCK - 1) // SAMPLES_PER_BLOCK
    C = SAMPLES_PER_BLOCK if mutate == "eight_call" else CALLS_PER_BLOCK
    i = np.arange(D, dtype=U64).reshape(1, 1, 1, D)
    j = np.arange(J, dtype=U64).reshape(J, 1, 1, 1)
    z = np.arange(Z, dtype=U64).reshape(1, Z, 1, 1)
    off = np.array([(int(offset) + c) & 0xFFFFFFFFFFFFFFFF for c in range(C)], dtype=U64).reshape(1, 1, C, 1)
    shape = (J, Z, C, D)
    c0 = np.broadcast_to(i, shape).astype(U32)
    c1 = np.broadcast_to((j << U64(16)) | z, shape).astype(U32)
    c2 = np.broadcast_to(off & U64(MASK32), shape).astype(U32)
    c3 = np.broadcast_to(off >> U64(32), shape).astype(U32)
    if mutate == "swap_words":
        c0, c1 = c1, c0
    return c0, c1, c2, c3


def eps_reference(seed, offset, J, S, D, mutate=None):
    """(eps, rad), float64 (J, S, D): the standard normals whvi_reparam_kl_philox_f32 draws at state = {seed, offset} and the
    Box-Muller radius of each.  Element i of matrix j, sample k: z = k // 8, q = k % 8, call = q // 4; counter
    (i, j << 16 | z, low32(offset + call), high32(offset + call)); key (low32(seed), high32(seed)); the four output words
    x0..x3 give the normals q % 4 = 0..3 as rad(x0) cos(x1), rad(x0) sin(x1), rad(x2) cos(x3), rad(x2) sin(x3) with
    u = uniform24(x), rad = sqrt(-2 log u), angle = float32(2 pi) * u in float32."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c = counters(offset, J, S, D, mutate)
    Z, C = c[0].shape[1:3]
    x = philox4x32_10(*c, U32(seed & MASK32), U32(seed >> 32))
    normals = np.empty((J, Z, C, 4, D), dtype=F64)
    radius = np.empty((J, Z, C, 4, D), dtype=F64)
    for p in range(2):
        u1, u2 = uniform24(x[2 * p]), uniform24(x[2 * p + 1])
        rad = np.sqrt(-2.0 * np.log(u1.astype(F64)))
        angle = (TWO_PI_F32 * u2).astype(F32).astype(F64)
        normals[:, :, :, 2 * p], normals[:, :, :, 2 * p + 1] = rad * np.cos(angle), rad * np.sin(angle)
        radius[:, :, :, 2 * p] = radius[:, :, :, 2 * p + 1] = rad
    if mutate == "eight_call":                 # sample q of a block takes the first normal of call q
        normals, radius = normals[:, :, :, 0], radius[:, :, :, 0]
    return (normals.reshape(J, Z * SAMPLES_PER_BLOCK, D)[:, :S].copy(), radius.reshape(J, Z * SAMPLES_PER_BLOCK, D)[:, :S].copy())


def counter_set(offset, J, S, D):
    """The launch's counters as one uint64 array of (c0, c1) and one of (c2, c3) per Philox call, flattened."""
    c0, c1, c2, c3 = counters(offset, J, S, D)
    return ((c1.astype(U64) << U64(32)) | c0.astype(U64)).ravel(), ((c3.astype(U64) << U64(32)) | c2.astype(U64)).ravel()


# ---- float64 closed forms with their yardsticks -----------------------------------------------------------------------------------
SOFTPLUS_THRESHOLD = 20.0
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)

ReparamKL = namedtuple("ReparamKL", "sigma u kl Y_kl")
ReparamKLBwd = namedtuple("ReparamKLBwd", "grad_mu grad_rho Y_mu Y_rho")
GaussMNLL = namedtuple("GaussMNLL", "loss grad_yhat grad_sigma Y_loss Y_yhat Y_sigma")


def _f32_scalar(v):
    """A Python float as the ABI receives it: rounded to float32, then held in float64."""
    return F64(F32(v))


def _softplus64(rho):
    rho = np.asarray(rho, dtype=F64)
    return np.where(rho > SOFTPLUS_THRESHOLD, rho, np.log1p(np.exp(np.minimum(rho, SOFTPLUS_THRESHOLD))))


def _softplus_slope64(rho):
    rho = np.asarray(rho, dtype=F64)
    return np.where(rho > SOFTPLUS_THRESHOLD, 1.0, 1.0 / (1.0 + np.exp(-rho)))


def reparam_kl_reference(mu, rho, eps, lam):
    """whvi_reparam_kl_f32 in float64: mu, rho (J, D), eps (J, S, D).  sigma = softplus(rho) in torch's threshold-20 form,
    u = [mu; sigma eps] (J, 1 + S, D), kl[j] = sum_i 0.5 (log lam - log sigma - 1 + sigma / lam + mu^2 / lam) and its yardstick
    Y_kl[j] = sum_i 0.5 (|log lam| + |log sigma| + 1 + sigma / lam + mu^2 / lam)."""
    mu, eps, lam = np.asarray(mu, dtype=F64), np.asarray(eps, dtype=F64), _f32_scalar(lam)
    sigma = _softplus64(rho)
    u = np.concatenate((mu[:, None, :], sigma[:, None, :] * eps), axis=1)
    kl = 0.5 * (np.log(lam) - np.log(sigma) - 1.0 + sigma / lam + mu * mu / lam).sum(axis=1)
    Y_kl = 0.5 * (abs(np.log(lam)) + np.abs(np.log(sigma)) + 1.0 + sigma / lam + mu * mu / lam).sum(axis=1)
    return ReparamKL(sigma, u, kl, Y_kl)


def reparam_kl_bwd_reference(gu, gk, mu, rho, eps, lam):
    """whvi_reparam_kl_bwd_f32 in float64: gu (J, 1 + S, D) and gk (J,) are the incoming gradients (either may be None = zero).
        grad_mu  = gu[:, 0] + gk mu / lam                                               Y_mu  = |gu[:, 0]| + |gk mu / lam|
        grad_rho = (sum_k gu[:, 1 + k] eps[:, k] + gk 0.5 (1 / lam - 1 / sigma)) s'     Y_rho = (sum_k |gu eps| + |gk| 0.5 (1 / lam + 1 / sigma)) s'
    with s' = sigmoid(rho), 1 above the threshold."""
    mu, eps, lam = np.asarray(mu, dtype=F64), np.asarray(eps, dtype=F64), _f32_scalar(lam)
    sigma, slope = _softplus64(rho), _softplus_slope64(rho)
    k = np.zeros(mu.shape[0]) if gk is None else np.asarray(gk, dtype=F64)
    k = k[:, None]
    grad_mu, Y_mu = k * mu / lam, np.abs(k * mu / lam)
    dsg, Y_sg = k * 0.5 * (1.0 / lam - 1.0 / sigma), np.abs(k) * 0.5 * (1.0 / lam + 1.0 / sigma)
    if gu is not None:
        gu = np.asarray(gu, dtype=F64)
        grad_mu, Y_mu = grad_mu + gu[:, 0], Y_mu + np.abs(gu[:, 0])
        dsg, Y_sg = dsg + (gu[:, 1:] * eps).sum(axis=1), Y_sg + np.abs(gu[:, 1:] * eps).sum(axis=1)
    return ReparamKLBwd(grad_mu, dsg * slope, Y_mu, Y_sg * slope)


def gauss_mnll_reference(y, y_hat, sigma, scale, g):
    """whvi_gauss_mnll_f32 and its backward in float64 on dense arrays of the broadcast shape; z = (y - y_hat) / sigma.
        loss       = scale sum(-0.5 z^2 - log sigma - 0.5 log 2 pi)        Y_loss  = |scale| sum(0.5 z^2 + |log sigma| + 0.5 log 2 pi)
        grad_yhat  = g scale (y - y_hat) / sigma^2                         Y_yhat  = |g scale| / sigma^2 (|y| + |y_hat|)
        grad_sigma = g scale (sum z^2 - count) / sigma                     Y_sigma = |g scale| / sigma (sum z^2 + count)"""
    y, y_hat = np.asarray(y, dtype=F64), np.asarray(y_hat, dtype=F64)
    sigma, scale, g = _f32_scalar(sigma), _f32_scalar(scale), _f32_scalar(g)
    z = (y - y_hat) / sigma
    zz, count = float((z * z).sum()), y_hat.size
    loss = scale * (-0.5 * zz - count * (np.log(sigma) + HALF_LOG_2PI))
    Y_loss = abs(scale) * (0.5 * zz + count * (abs(np.log(sigma)) + HALF_LOG_2PI))
    gs = g * scale
    return GaussMNLL(loss, gs * (y - y_hat) / sigma ** 2, gs * (zz - count) / sigma,
                     Y_loss, abs(gs) / sigma ** 2 * (np.abs(y) + np.abs(y_hat)), abs(gs) / sigma * (zz + count))


# ---- the bounds of tests/test_train_aux_gpu.py ------------------------------------------------------------------------------------
# multiples of the yardstick (sigma: of the reference itself; eps: of |reference| plus a floor); u is compared bit for bit
BOUNDS = {"sigma": 1e-6, "kl": 2e-6, "grad_mu": 2e-6, "grad_rho": 2e-6, "eps": 2e-6, "loss": 2e-6, "grad_yhat": 1e-6, "grad_sigma": 2e-6}
EPS_FLOOR = 1e-7


def worst_ratio(got, ref, yardstick, bound, floor=0.0):
    """max over elements of |got - ref| / (bound * yardstick + floor); 0 / 0 counts as 0, anything else over 0 and any
    non-finite value as inf.  At most 1 means every element is inside its bound."""
    got, ref = np.asarray(got, dtype=F64), np.asarray(ref, dtype=F64)
    err, lim = np.abs(got - ref), bound * np.asarray(yardstick, dtype=F64) + floor
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / lim)
    ratio = np.where(np.isfinite(got) & np.isfinite(ratio), ratio, np.inf)
    return float(ratio.max())


# ---- float32 emulations of the kernels --------------------------------------------------------------------------------------------
def _block_sum_256(v):
    """v (..., 256) float32 -> (...): the 64-lane shuffle tree of each wave (lane l += lane l + off, off = 32 .. 1), then
    (wave 0 + wave 1) + (wave 2 + wave 3), as lane 0 / thread 0 sees it."""
    w = v.reshape(v.shape[:-1] + (4, 64)).astype(F32)
    for off in (32, 16, 8, 4, 2, 1):
        w = (w[..., :off] + w[..., off:2 * off]).astype(F32)
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]).astype(F32) + (w[..., 2] + w[..., 3]).astype(F32)).astype(F32)


def _softplus32(rho, mutate=None):
    rho = np.asarray(rho, dtype=F32)
    e = np.exp(np.minimum(rho, F32(SOFTPLUS_THRESHOLD))).astype(F32)
    with np.errstate(divide="ignore"):
        soft = np.log(F32(1.0) + e).astype(F32) if mutate == "naive_log" else np.log1p(e).astype(F32)
    return np.where(rho > F32(SOFTPLUS_THRESHOLD), rho, soft).astype(F32)


def emulate_reparam_kl(mu, rho, eps, lam, mutate=None):
    """reparam_kl_kernel (and the Philox kernel behind its draw) in float32: (sigma, u, kl).  ``mutate="naive_log"``:
    log(1 + exp(rho)) in place of log1p(exp(rho))."""
    mu, eps, lam = np.asarray(mu, dtype=F32), np.asarray(eps, dtype=F32), F32(lam)
    J, D = mu.shape
    sg = _softplus32(rho, mutate)
    u = np.concatenate((mu[:, None, :], (sg[:, None, :] * eps).astype(F32)), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.log(lam) - np.log(sg)
        term = (term - F32(1.0)).astype(F32)
        term = (term + (sg / lam).astype(F32)).astype(F32)
        term = (F32(0.5) * (term + (mu * (mu / lam).astype(F32)).astype(F32)).astype(F32)).astype(F32)
    nblk = (D + 255) // 256
    padded = np.zeros((J, nblk * 256), dtype=F32)
    padded[:, :D] = term
    part = _block_sum_256(padded.reshape(J, nblk, 256))
    kl = part[:, 0].copy()
    for b in range(1, nblk):                   # _hip.reparam_kl: part.sum(dim=1)
        kl = (kl + part[:, b]).astype(F32)
    return sg, u, kl


def emulate_reparam_kl_bwd(gu, gk, mu, rho, eps, sigma, lam, mutate=None):
    """reparam_kl_bwd_kernel in float32 on the forward's float32 sigma: (grad_mu, grad_rho).  ``mutate="drop_last_sample"``:
    the sample loop stops one sample early; ``"sigmoid_everywhere"``: the slope is sigmoid(rho) above the threshold too."""
    mu, rho, eps, sg, lam = (np.asarray(v, dtype=F32) for v in (mu, rho, eps, sigma, lam))
    J, D = mu.shape
    S = eps.shape[1]
    k = np.zeros((J, 1), dtype=F32) if gk is None else np.asarray(gk, dtype=F32)[:, None]
    one, half = F32(1.0), F32(0.5)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dmu = (k * (mu / lam).astype(F32)).astype(F32)
        dsg = (k * (half * ((one / lam).astype(F32) - (one / sg).astype(F32)).astype(F32)).astype(F32)).astype(F32)
        if gu is not None:
            gu = np.asarray(gu, dtype=F32)
            dmu = (dmu + gu[:, 0]).astype(F32)
            acc = np.zeros((J, D), dtype=F32)
            for s in range(S - 1 if mutate == "drop_last_sample" else S):
                acc = (acc + (gu[:, s + 1] * eps[:, s]).astype(F32)).astype(F32)
            dsg = (dsg + acc).astype(F32)
        slope = (one / (one + np.exp(-rho).astype(F32)).astype(F32)).astype(F32)
        scaled = (dsg * slope).astype(F32)
    grad_rho = scaled if mutate == "sigmoid_everywhere" else np.where(rho > F32(SOFTPLUS_THRESHOLD), dsg, scaled)
    return dmu, grad_rho.astype(F32)


def mnll_blocks(total):
    """train_aux.hip: mnll_blocks -- about four elements per thread, at most 2048 blocks."""
    return min(max((total + 1023) // 1024, 1), 2048)


def emulate_gauss_mnll(y, y_hat, sigma, scale, g, mutate=None):
    """gauss_mnll_kernel, the float32 sum of its partial sums, and gauss_mnll_bwd_kernel: (loss, grad_yhat, grad_sigma).  y and
    y_hat are float32 arrays of the broadcast shape IN THE ORDER THE KERNEL WALKS THEM (y_hat's memory order); grad_yhat comes
    back in that order.  ``mutate="no_count"``: grad_sigma without ``- count``."""
    y, yh = np.asarray(y, dtype=F32).ravel(), np.asarray(y_hat, dtype=F32).ravel()
    sg, scale, g = F32(sigma), F32(scale), F32(g)
    total, blocks = yh.size, mnll_blocks(yh.size)
    threads = blocks * 256
    inv = F32(F32(1.0) / sg)
    cst = F32(np.log(sg).astype(F32) + F32(HALF_LOG_2PI))
    acc_ld, acc_zz = np.zeros(threads, dtype=F32), np.zeros(threads, dtype=F32)
    for start in range(0, total, threads):                       # one trip of the grid-stride loop
        n = min(threads, total - start)
        z = ((y[start:start + n] - yh[start:start + n]).astype(F32) * inv).astype(F32)
        zz = (z * z).astype(F32)
        acc_zz[:n] = (acc_zz[:n] + zz).astype(F32)
        acc_ld[:n] = (acc_ld[:n] + ((F32(-0.5) * zz).astype(F32) - cst).astype(F32)).astype(F32)
    part_ld = (scale * _block_sum_256(acc_ld.reshape(blocks, 256))).astype(F32)
    part_zz = _block_sum_256(acc_zz.reshape(blocks, 256))
    loss = F32(part_ld[0]) if blocks == 1 else F32(np.sum(part_ld, dtype=F32))
    # backward
    gs = F32(g * scale)
    w = F32(gs / F32(sg * sg))
    grad_yhat = (w * (y - yh).astype(F32)).astype(F32)
    per_thread = np.zeros(256, dtype=F32)
    for start in range(0, blocks, 256):
        n = min(256, blocks - start)
        per_thread[:n] = (per_thread[:n] + part_zz[start:start + n]).astype(F32)
    zz = _block_sum_256(per_thread)
    centred = zz if mutate == "no_count" else F32(zz - F32(total))
    return loss, grad_yhat, F32(F32(gs * centred) / sg)


# ---- the case list ----------------------------------------------------------------------------------------------------------------
J_CASES = 2
RHO_RANGE = 30.0                                   # rho uniform in [-30, 30]: 1 / sigma and exp(-rho) stay finite in float32
LAMBDAS = (1e-5, 0.37, 50.0)
FWD_D = (1, 255, 256, 257, 700)                    # a partial block, an exact block, more than one KL partial
FWD_S = (0, 1, 8, 9, 21)                           # blockIdx.z = 0, 1, 2, the last one partial
FWD_CASES = tuple({"id": f"D{D}-S{S}-lam{lam:g}", "J": J_CASES, "D": D, "S": S, "lam": lam}
                  for D, S, lam in itertools.product(FWD_D, FWD_S, LAMBDAS))

# the same grid thinned: S around the sample loop's unroll of four, every D, every lambda, the three gradient combinations
_BWD = ((1, 0, 0.37, "both"), (1, 3, 1e-5, "both"), (255, 4, 50.0, "both"), (256, 5, 1e-5, "both"), (257, 9, 0.37, "both"),
        (700, 3, 1e-5, "both"), (700, 9, 50.0, "both"), (257, 5, 50.0, "both"), (257, 4, 1e-5, "kl_only"),
        (700, 0, 0.37, "kl_only"), (255, 5, 0.37, "u_only"), (700, 9, 1e-5, "u_only"), (256, 3, 50.0, "u_only"))
BWD_CASES = tuple({"id": f"D{D}-S{S}-lam{lam:g}-{grads}", "J": J_CASES, "D": D, "S": S, "lam": lam, "grads": grads}
                  for D, S, lam, grads in _BWD)

PHILOX_SHAPES = ((1, 1, 1), (2, 8, 256), (3, 21, 1000), (2, 9, 257), (2, 0, 5))
PHILOX_SEEDS = (1234, 0x123456789ABCDEF0)          # the second: both key words non-zero
PHILOX_OFFSETS = (0, 2 ** 32 - 1)                  # the second: the block's second call carries into the high counter word
PHILOX_CASES = tuple({"id": f"J{J}-S{S}-D{D}-seed{seed:x}-off{off:x}", "J": J, "S": S, "D": D, "seed": seed, "offset": off}
                     for (J, S, D), seed, off in itertools.product(PHILOX_SHAPES, PHILOX_SEEDS, PHILOX_OFFSETS))

MNLL_SHAPES = ((100, 1, 1, "perm"), (37, 3, 5, "perm"), (64, 2, 8, "contig"), (1, 1, 1, "contig"), (5000, 1, 64, "perm"),
               (9, 4, 3, "expand"),
               (33000, 1, 64, "perm"),             # 2 112 000 elements: past 2048 blocks x 1024, every thread loops
               (40, 3, 5, "gaps"))                 # the first three of five outputs of a permuted buffer
MNLL_SIGMAS = (0.05, 0.7, 30.0)
MNLL_RESIDUALS = ("normal", "calibrated")          # y_hat ~ N(0, 1) beside y ~ N(0, 1);  y_hat = y + sigma N(0, 1)
MNLL_WIDE = 5                                      # "gaps": outputs of the buffer the view is cut from
MNLL_N, MNLL_G = 4321, -1.7                        # data-set size in scale = -n / (m n_mc); incoming gradient
MNLL_CASES = tuple({"id": f"m{m}-o{o}-mc{mc}-{layout}-sigma{sg:g}-{res}", "m": m, "n_out": o, "n_mc": mc, "layout": layout,
                    "sigma": sg, "residuals": res}
                   for (m, o, mc, layout), sg, res in itertools.product(MNLL_SHAPES, MNLL_SIGMAS, MNLL_RESIDUALS))


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def reparam_inputs(case, with_eps=True):
    """Seeded float32 inputs of a forward or backward case: mu ~ 0.5 N(0, 1); rho uniform in [-30, 30] with the first entries of
    each row at the threshold, one float above it and one below; eps, gu, gk ~ N(0, 1) (gu / gk None as case["grads"] says)."""
    J, D, S = case["J"], case["D"], case["S"]
    rng = _rng(J, D, S, round(case["lam"] * 1e6))
    mu = (0.5 * rng.standard_normal((J, D))).astype(F32)
    rho = rng.uniform(-RHO_RANGE, RHO_RANGE, (J, D)).astype(F32)
    t = F32(SOFTPLUS_THRESHOLD)
    edge = np.array([t, np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(0.0))], dtype=F32)
    rho[:, :3] = edge[:min(D, 3)]
    out = {"mu": mu, "rho": rho, "lam": case["lam"]}
    if with_eps:
        out["eps"] = rng.standard_normal((J, S, D)).astype(F32)
    grads = case.get("grads")
    if grads is not None:
        gu, gk = rng.standard_normal((J, S + 1, D)).astype(F32), rng.standard_normal(J).astype(F32)
        out["gu"], out["gk"] = (gu if grads != "kl_only" else None), (gk if grads != "u_only" else None)
    return out


def mnll_inputs(case):
    """Seeded float32 inputs of an MNLL case.  ``base`` is the buffer the predictions live in and ``view(base)`` their
    (m, n_out, n_mc) view (numpy or torch: permute / slicing only); ``y`` (m, n_out).  ``walk(a)`` puts an (m, n_out, n_mc)
    array into the order the kernel walks the elements (decreasing y_hat stride)."""
    m, o, mc, layout = case["m"], case["n_out"], case["n_mc"], case["layout"]
    rng = _rng(m, o, mc, round(case["sigma"] * 100), MNLL_RESIDUALS.index(case["residuals"]))
    sigma = F32(case["sigma"])
    y = rng.standard_normal((m, o)).astype(F32)
    noise = rng.standard_normal((m, o, mc)).astype(F32)
    dense = noise if case["residuals"] == "normal" else (y[:, :, None] + sigma * noise).astype(F32)
    if layout == "expand":                       # a network without stochastic layers: one prediction, expanded, made contiguous
        dense = np.ascontiguousarray(np.broadcast_to(dense[:, :, :1], (m, o, mc)))
    if layout in ("contig", "expand"):
        base, walk = dense.copy(), (lambda a: a)
        view = (lambda t: t)
    elif layout == "perm":                       # what forward_batched returns: (n_mc, m, n_out) permuted
        base, walk = np.ascontiguousarray(dense.transpose(2, 0, 1)), (lambda a: a.transpose(2, 0, 1))
        view = (lambda t: t.transpose(1, 2, 0) if isinstance(t, np.ndarray) else t.permute(1, 2, 0))
    else:                                        # "gaps": the first n_out of MNLL_WIDE outputs of such a buffer
        base = rng.standard_normal((mc, m, MNLL_WIDE)).astype(F32)
        base[:, :, :o] = dense.transpose(2, 0, 1)
        walk = (lambda a: a.transpose(2, 0, 1))
        view = (lambda t: (t.transpose(1, 2, 0) if isinstance(t, np.ndarray) else t.permute(1, 2, 0))[:, :o, :])
    return {"y": y, "base": base, "view": view, "walk": walk, "dense": dense, "sigma": float(sigma),
            "scale": -MNLL_N / (m * mc), "g": MNLL_G}


if __name__ == "__main__":
    for name, cases in (("reparam_kl", FWD_CASES), ("reparam_kl_bwd", BWD_CASES), ("reparam_kl_philox", PHILOX_CASES),
                        ("gauss_mnll", MNLL_CASES)):
        print(f"{name}: {len(cases)} cases")
        for c in cases:
            print("   ", c["id"])
