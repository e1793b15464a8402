"""The float64 yardsticks of csrc/bn.hip -- the BatchNorm finalize kernels, the ResBlock tail and its backward reductions, and the
power-of-two gradient scales of the f16 split kernels -- with the case tables, the input builders and the bounds, for
tests/test_gpu_bn_stack.py (GPU) and tests/test_bn_yardstick_cpu.py (the same bounds met by a float32 restatement of every kernel's
formula, the input margins, and the restatements with a defect planted, without a GPU).  `import bn_yardstick as Y`.  Numpy alone, but
for the producer chain (section G), which runs the oracle's ResBlock in torch.

Bounds.  Every kernel here is a short, known chain of float32 or float64 operations, so every bound is derived, per element, from
U = 2^-24, gamma(n) and ulp32 of the float64 reference; none takes a number from a kernel.  The derivation stands next to each table.
A value the kernel computes in double and rounds once to float32 is held to 1 ulp32 (half an ulp of rounding; the other half covers
the kernel's own double round-off, which the conditioning of E[x^2] - E[x]^2 can lift well above 2^-53).

Partials.  wm_bn_finalize and wm_bn_bwd_finalize are given float32 partial sums built here, and the reference is float64 arithmetic on
those same partials: their producers' round-off is not charged.  The tables keep the partials of a channel on one power-of-two grid
(sum_exact asserts it), so that their double sum is exact in any order -- the kernel's sixteen slices included.

Restatements.  `*_restated` functions repeat a kernel's formula with numpy in the kernel's own number formats; `defect=` plants one of
the defects the tests must notice.  fmaf(b, sc, sh) is restated as the product in double (exact: 24 x 24 bits) plus sh, rounded once to
float32 -- double rounding can differ from the fused operation by less than 2^-29 ulp.

Measured on 1 x MI355X, the largest |kernel - float64| / bound of any compared element, per kernel (tests/test_gpu_bn_stack.py prints
every figure):

    wm_bn_finalize              scale, shift, save_mean, save_invstd, running_mean, running_var        0.50
    wm_bn_eval_scale_shift      scale, shift                                                           0.65
    wm_bn_add_relu(_mask)       out (the mask: bit for bit)                                            0.50
    wm_relu_bwd_reduce(_mask)   partial (dz, dzmax: bit for bit)                                       0.43 (T = 4); 0.015 at T >= 4092
    wm_bn_bwd_finalize          A, C, dgamma, dbeta 0.68; zero-sum residue / (2^-45 of its terms)      0.03
    wm_gscale_absmax, wm_gscale_from_max, wm_absmax_rows: exact (the scale is the one power of two of the interval)
    producer chain              |mean| / std 0 and 3: every tensor within 0.07 of its bar; 30: see below

Findings.  (1) Fixed with this file: the scale kernels computed exp2f(floorf(L - log2f(m))), which for a maximum just above a power of
two gives a scale one binade too large (m = nextafter(2^-20), L = 9: max |x| gs = 512.00006; section F and the CPU file's comparison of
the two formulas).  They now take the exponent of m itself.  (2) Measured, not fixed (the convolution epilogues are out of this file's
reach): at |mean| / std = 30 the ResBlock's output is 3.5 x (1, 64) and 1.6 x (3, 132) its bar from float64, BN2's new running mean
2.3 x and 1.6 x, where the float32 oracle is at 0.1 -- kept as strict expected failures in tests/test_gpu_bn_stack.py.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from loss_yardstick import bar, held, rel_err  # noqa: F401  (the rule max(8 * e32, floor); re-exported for the two test files)
from oracle import wm_oracle as O
from yardstick_common import U, gamma, ulp32

TINY = 2.0 ** -149
F32 = np.float32


def rng(seed):
    return np.random.default_rng(seed)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def sum_exact(partials):
    """the [nparts][2][64] partials summed over the parts in float64, and whether that sum is exact (equal to the long double one)"""
    s = f64(partials).sum(axis=0)
    sl = np.asarray(partials, dtype=np.longdouble).sum(axis=0)
    return s, bool(np.all(sl == s.astype(np.longdouble)))


# --------------------------------------------------------------------------------------------------------------- A. wm_bn_finalize
# mean = s1 / count, var = max(s2 / count - mean^2, 0), invstd = 1 / sqrt(var + eps), all in double from double sums of the partials;
# scale = (float)(gamma invstd), shift = (float)(beta - mean gamma invstd), save_mean, save_invstd, and the running statistics
# (1 - momentum) r + momentum (mean | var count / (count - 1)) are each rounded once: 1 ulp32 of the reference, plus the spacing of
# float32's denormals.  momentum and eps are the float32 values the kernel receives.
MOMENTUM, EPS = float(F32(0.1)), float(F32(1e-5))
NBT_START = (1 << 32) + 5                       # num_batches_tracked before the launch: the += 1 must carry into the high word
FIN_NPARTS = (1, 15, 16, 17, 256, 1000)
CH_CONST, CH_GAMMA0, CH_GAMMANEG, CH_OFFCENTRE = 3, 7, 11, 19       # the channels of a launch that are not ordinary
# (name, nparts, elements per part and channel, running statistics given)
FIN_CASES = [(f"nparts{n}", n, 64, True) for n in FIN_NPARTS] + [
    ("count1", 1, 1, True),                     # count == 1: the unbiased variance falls back to the biased one
    ("norunning", 17, 64, False),               # running_mean == NULL: scale / shift written, running buffers and the counter untouched
    ("bigcount", 256, 16000, True),             # count = 256 * 16000, a training step's
]
FIN_NAMES = ("scale", "shift", "save_mean", "save_invstd", "running_mean", "running_var")


def _odd_part(n):
    return n // (n & -n)


def finalize_inputs(nparts, per_part, seed=0):
    """partials [nparts][2][64] float32 of per_part elements per part and channel, gamma, beta, running_mean, running_var (float32) and
    the count.  A part holds up to 8 drawn values, each standing for the same number of elements; values and weights sit on
    power-of-two grids, so the partials of a channel are exact float32 numbers whose double sum is exact.
    CH_CONST: every element is 30, and every s2 partial is rounded one float32 step down, so that s2 / count - mean^2 < 0 by some
    5e-5, five times eps (without the clamp: the root of a negative number).  CH_OFFCENTRE: |mean| / std = 100."""
    r = rng(1000 + 7 * nparts + per_part + seed)
    # the weight of a draw is a power of two times an odd number below 32, so that a weighted sum of squares keeps to 24 bits
    draws = next(d for d in range(min(per_part, 8), 0, -1) if per_part % d == 0 and _odd_part(per_part // d) < 32)
    w = per_part // draws
    mu, sd = r.uniform(-1.0, 1.0, 64), r.uniform(0.25, 1.5, 64)
    mu[CH_OFFCENTRE], sd[CH_OFFCENTRE] = 12.5, 0.125
    x = mu[None, None, :] + sd[None, None, :] * r.standard_normal((nparts, draws, 64))
    x = np.clip(np.round(x * 16.0) / 16.0, -15.0, 15.0)           # 2^-4 grid, |x| < 16: x^2 on the 2^-8 grid, below 2^8
    x[:, :, CH_CONST] = 30.0
    s1, s2 = w * x.sum(axis=1), w * (x * x).sum(axis=1)
    part = np.stack([s1, s2], axis=1)
    assert np.all(f32(part).astype(np.float64) == part), "a partial is no float32 number"
    part = f32(part)
    if per_part > 1:
        part[:, 1, CH_CONST] = np.nextafter(part[:, 1, CH_CONST], F32(0))
    gam, bet = f32(r.uniform(0.5, 1.5, 64)), f32(r.uniform(-0.5, 0.5, 64))
    gam[CH_GAMMA0], gam[CH_GAMMANEG] = 0.0, -1.25
    return dict(partials=part, gamma=gam, beta=bet, running_mean=f32(r.uniform(-0.5, 0.5, 64)), running_var=f32(r.uniform(0.5, 2.0, 64)),
                count=float(nparts * per_part))


def finalize_ref(inp, running=True, defect=None, sums=None):
    """float64: {scale, shift, save_mean, save_invstd, running_mean, running_var, var_raw}.  defect (for the restatement):
    "no_clamp" drops var < 0 -> 0, "biased" feeds the biased variance to running_var."""
    s = sum_exact(inp["partials"])[0] if sums is None else sums
    n = inp["count"]
    mean = s[0] / n
    raw = s[1] / n - mean * mean
    var = raw if defect == "no_clamp" else np.maximum(raw, 0.0)
    with np.errstate(invalid="ignore"):
        invstd = 1.0 / np.sqrt(var + EPS)
    ga, be = f64(inp["gamma"]), f64(inp["beta"])
    out = dict(scale=ga * invstd, shift=be - mean * ga * invstd, save_mean=mean, save_invstd=invstd, var_raw=raw)
    if running:
        unb = var * n / (n - 1.0) if n > 1.0 and defect != "biased" else var
        out["running_mean"] = (1.0 - MOMENTUM) * f64(inp["running_mean"]) + MOMENTUM * mean
        out["running_var"] = (1.0 - MOMENTUM) * f64(inp["running_var"]) + MOMENTUM * unb
    else:
        out["running_mean"], out["running_var"] = f64(inp["running_mean"]), f64(inp["running_var"])
    return out


def finalize_restated(inp, running=True, defect=None):
    """the kernel's formula: sixteen slices p = j, j + 16, ... summed in double one after the other, the slices added in order, the
    formula in double, every output rounded to float32"""
    part = f64(inp["partials"])
    sl = np.zeros((16, 2, 64))
    for j in range(16):
        for q in range(j, part.shape[0], 16):
            sl[j] += part[q]
    s = np.zeros((2, 64))
    for j in range(16):
        s += sl[j]
    ref = finalize_ref(inp, running, defect, sums=s)
    return {k: f32(v) for k, v in ref.items()}


def finalize_bound(ref, name):
    return ulp32(ref[name]) + TINY


# ------------------------------------------------------------------------------------------------------- B. wm_bn_eval_scale_shift
# Four float32 operations: v = rv + eps (U), r = sqrtf(v) (halves what v carries, + U), inv = 1 / r (+ U): inv within 2.5 U;
# scale = gamma inv (+ U): 3.5 U |scale|.  shift = beta - (rm gamma) inv: the product rm gamma (U), times inv (2.5 U + U, or none where
# the compiler fuses it into the subtraction): 4.5 U |rm gamma inv|, and the subtraction's own rounding U |shift|.  Stated with whole
# numbers: 4 U |scale|; 5 U |rm gamma inv| + U |shift|.
EVAL_RV = (0.0, 1e-12, 1.0, 1e6)


def eval_inputs():
    """64 channels: running_var cycles through EVAL_RV; gamma negative on every third channel; |running_mean| up to 1e4"""
    r = rng(77)
    c = np.arange(64)
    rv = f32(np.array(EVAL_RV)[c % 4])
    gam = f32(r.uniform(0.5, 1.5, 64) * np.where(c % 3 == 0, -1.0, 1.0))
    rm = f32(r.uniform(-1.0, 1.0, 64) * np.array([1.0, 1e2, 1e4, 1e-3])[(c // 4) % 4])
    return dict(gamma=gam, beta=f32(r.uniform(-0.5, 0.5, 64)), running_mean=rm, running_var=rv)


def eval_ref(inp):
    inv = 1.0 / np.sqrt(f64(inp["running_var"]) + EPS)
    t = f64(inp["running_mean"]) * f64(inp["gamma"]) * inv
    return dict(scale=f64(inp["gamma"]) * inv, shift=f64(inp["beta"]) - t, term=t)


def eval_restated(inp):
    inv = F32(1.0) / np.sqrt(inp["running_var"] + F32(EPS), dtype=np.float32)
    return dict(scale=inp["gamma"] * inv, shift=inp["beta"] - inp["running_mean"] * inp["gamma"] * inv)


def eval_bound(ref, name):
    if name == "scale":
        return 4 * U * np.abs(ref["scale"]) + TINY
    return 5 * U * np.abs(ref["term"]) + U * np.abs(ref["shift"]) + TINY


# --------------------------------------------------------------------------------- C. wm_bn_add_relu, wm_bn_add_relu_mask (the tail)
# out = fmaxf(x + fmaf(y, sc, sh), 0): the fused multiply-add is within half an ulp32 of t = y sc + sh, the sum within half an ulp32
# of itself, fmaxf is exact: ulp32(t) + ulp32(out) covers both with room for the ulp of the reference standing for the ulp of the
# computed value.  Where the float64 r = x + y sc + sh is <= 0 the kernel must give +0.0 and a clear bit, which is decidable only if no
# |r| is within round-off of 0: every |r| is at least MARGIN_ULPS ulp32 of its largest term (tail_inputs sees to it, tail_margin
# measures it), except the planted exact zeros (x = y = sh = 0: r = 0 in any arithmetic, bit 0).
# T in float4 units: 1, 7, 8, 9 (around one mask dword), 1023, 1024, 1025 (around one unrolled iteration of 256 threads x 4), 2049.
TAIL_T = (4, 28, 32, 36, 4092, 4096, 4100, 8196)
TAIL_B = (1, 3)
MARGIN_ULPS = 64
CH_ZEROS = 5                                    # shift 0 and exact zeros in x and y at every 7th step
CANARY = 8                                      # untouched elements on either side of every output


def tail_inputs(B, T):
    """x, y [B, 64, T], scale, shift [64] float32, a different scale (both signs) and shift for every channel"""
    r = rng(300 + 11 * B + T)
    x, y = f32(r.standard_normal((B, 64, T))), f32(r.standard_normal((B, 64, T)))
    sc = f32(r.uniform(0.5, 1.5, 64) * np.where(np.arange(64) % 4 == 1, -1.0, 1.0))
    sh = f32(r.uniform(-0.5, 0.5, 64))
    sh[CH_ZEROS] = 0.0
    for t in planted_steps(T):                  # the backward's planted maxima need a set bit there
        x[:, :, t] = np.abs(f64(y[:, :, t]) * sc[None, :] + sh[None, :]) + 1.0
    x[:, CH_ZEROS, ::7] = 0.0
    y[:, CH_ZEROS, ::7] = 0.0
    for _ in range(8):
        bad = ~tail_margin_ok(x, y, sc, sh)
        if not bad.any():
            break
        x[bad] += F32(0.5)
    return x, y, sc, sh


def tail_terms(x, y, sc, sh):
    """float64: t = y sc + sh, r = x + t, and the largest of |x|, |y sc|, |sh| per element"""
    ys = f64(y) * f64(sc)[None, :, None]
    t = ys + f64(sh)[None, :, None]
    big = np.maximum(np.maximum(np.abs(f64(x)), np.abs(ys)), np.abs(f64(sh))[None, :, None])
    return t, f64(x) + t, big


def tail_margin_ok(x, y, sc, sh):
    t, r, big = tail_terms(x, y, sc, sh)
    return (np.abs(r) >= MARGIN_ULPS * ulp32(big)) | (big == 0.0)


def tail_ref(x, y, sc, sh):
    """(out float64, positive bool, bound)"""
    t, r, _ = tail_terms(x, y, sc, sh)
    out = np.maximum(r, 0.0)
    return out, r > 0.0, ulp32(t) + ulp32(out)


def pack_mask(pos):
    """bool [B, 64, T] -> uint32 [B * 64, ceil(T / 32)]: bit t % 32 of dword t / 32, the bits past T clear"""
    B, C, T = pos.shape
    nw = (T + 31) // 32
    padded = np.zeros((B * C, nw * 32), dtype=np.uint64)
    padded[:, :T] = pos.reshape(B * C, T)
    return (padded.reshape(B * C, nw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack_mask(mask, T):
    """uint32 [rows, nw] -> bool [rows, T]"""
    b = (mask[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return b.reshape(mask.shape[0], -1)[:, :T].astype(bool)


def tail_restated(x, y, sc, sh, defect=None):
    """(out float32, mask uint32).  defect: "row_mod_B" takes the channel as row % B instead of row & 63, "mask_shift" shifts every mask
    dword up by one bit"""
    B = x.shape[0]
    if defect == "row_mod_B":
        c = (np.arange(B * 64) % B).reshape(B, 64)
        scr, shr = sc[c][:, :, None], sh[c][:, :, None]
    else:
        scr, shr = sc[None, :, None], sh[None, :, None]
    t = f32(f64(y) * f64(scr) + f64(shr))
    out = np.maximum(x + t, F32(0.0))
    mask = pack_mask(out > 0)
    if defect == "mask_shift":
        mask = (mask << np.uint32(1)).astype(np.uint32)
    return out, mask


# --------------------------------------------------------------------------- D. wm_relu_bwd_reduce, wm_relu_bwd_reduce_mask (backward)
# dz = g where the bit is set, else +0.0: exact.  dzmax[row] = max |dz|: exact.  partial[b][0][c] = sum_t dz and partial[b][1][c] =
# sum_t dz y in float32: T terms in some order are T - 1 roundings, the products one more: gamma(T) sum |terms| for both.  At the long
# shapes that says little, so the bound is the smaller of it and gamma(depth) sum |terms| with the depth of the kernel's own summation:
# a term passes through its product, the fused multiply-add and the sum of its float4 (3 roundings), the ceil(T / 1024) additions of its
# thread's float4s (every 256th), six levels of the wave's butterfly and three additions across the four waves: ceil(T / 1024) + 12.
def planted_steps(T):
    """where a row's largest |g| is put, by row % 3: in the first quad, in the last quad (which is the last float4 of the ragged
    iteration where T / 4 is no multiple of 1024), and in the first float4 of that last iteration of the 256 x 4 x 4-element loop"""
    T4 = T // 4
    return (1, T - 2, 4 * (((T4 - 1) // 1024) * 1024) + 2)


def reduce_inputs(B, T, pos):
    """g [B, 64, T] float32 for the mask `pos` of tail_ref: unit normal; in every row the largest |g| of a set bit (10 + row / 100,
    negative on odd rows) at planted_steps(T)[row % 3], and a larger one, 20, under the first clear bit of every fourth row"""
    g = f32(rng(400 + 11 * B + T).standard_normal((B, 64, T)))
    g[:, :, 5 % T] = 0.0
    gr, pr = g.reshape(B * 64, T), pos.reshape(B * 64, T)
    steps = planted_steps(T)
    for row in range(B * 64):
        t = steps[row % 3]
        assert pr[row, t]
        gr[row, t] = (10.0 + row / 100.0) * (-1.0 if row & 1 else 1.0)
        off = np.flatnonzero(~pr[row])
        if row % 4 == 1 and off.size:
            gr[row, off[0]] = 20.0
    return g


def reduce_depth(T):
    """the largest number of roundings a term of the kernel's sums passes through"""
    return -(-T // 1024) + 12


def reduce_ref(g, y, pos):
    """(dz float32 exact, dzmax float32 [B * 64] exact, partial float64 [B, 2, 64], bound [B, 2, 64])"""
    B, _, T = g.shape
    dz = np.where(pos, g, F32(0.0)).astype(np.float32)
    d, yy = f64(dz), f64(y)
    part = np.stack([d.sum(axis=2), (d * yy).sum(axis=2)], axis=1)
    bound = min(gamma(T), gamma(reduce_depth(T))) * np.stack([np.abs(d).sum(axis=2), np.abs(d * yy).sum(axis=2)], axis=1) + TINY
    return dz, np.abs(dz).max(axis=2).reshape(-1), part, bound


def reduce_restated(g, y, mask, defect=None):
    """(dz, dzmax, partial float32) from the packed mask, summed as the kernel's threads do: a float4's four terms pairwise, a thread's
    float4s (every 256th) one after the other, the 256 threads by halves"""
    B, _, T = g.shape
    pos = unpack_mask(mask, T).reshape(B, 64, T)
    dz = np.where(pos, g, F32(0.0)).astype(np.float32)
    T4 = T // 4
    it = -(-T4 // 256)

    def block(q):                               # q [B, 64, T4] float32, one value per float4
        pad = np.zeros((B, 64, it * 256), dtype=np.float32)
        pad[:, :, :T4] = q
        acc = np.zeros((B, 64, 256), dtype=np.float32)
        for i in range(it):
            acc = acc + pad[:, :, i * 256:(i + 1) * 256]
        while acc.shape[2] > 1:                 # the threads by halves: eight levels (the kernel: six in the wave, three across)
            half = acc.shape[2] // 2
            acc = acc[:, :, :half] + acc[:, :, half:]
        return acc[:, :, 0]
    d4, p4 = dz.reshape(B, 64, T4, 4), (dz * y).reshape(B, 64, T4, 4)
    s1 = block((d4[..., 0] + d4[..., 1]) + (d4[..., 2] + d4[..., 3]))
    s2 = block((p4[..., 0] + p4[..., 1]) + (p4[..., 2] + p4[..., 3]))
    return dz, np.abs(dz).max(axis=2).reshape(-1), np.stack([s1, s2], axis=1)


# ---------------------------------------------------------------------------------------------------------- E. wm_bn_bwd_finalize
# From double sums s1 = sum dz, s2 = sum dz y:  sxh = (s2 - mu s1) invstd;  A = (float)(gamma invstd);  C = (float)(-gamma invstd^2
# sxh / count);  dgamma = (float)sxh, dbeta = (float)s1: one rounding each, 1 ulp32; with accumulate the float32 sum prev + (float)v
# adds its own rounding: ulp32(v) + ulp32(prev + v).  eval_mode: C = 0 and B = 0 exactly.
# B = -(A s1 + C mu count) / count is formed in double from the ROUNDED A and C and handed over as Bhi + Blo, so that
# A s1 + (Bhi + Blo) count + C mu count vanishes: to ZERO_SUM = 2^-45 of the sum of the three magnitudes (Blo is rounded to float32:
# 2^-24 of a word that is at most 2^-24 of B, and a few double roundings), and |Blo| <= ulp32(Bhi) / 2.  The residue is evaluated from
# the kernel's own A, C, Bhi, Blo.  The partials sit on the 2^-10 grid below 2^10, so s1 and s2 are exact in any order.
BWD_NPARTS = (1, 16, 17, 300)
BWD_CASES = [(n, acc, ev) for n in BWD_NPARTS for acc in (0, 1) for ev in (0, 1)]
ZERO_SUM = 2.0 ** -45


def bwd_inputs(nparts, seed=0):
    r = rng(500 + nparts + seed)
    part = np.round(r.standard_normal((nparts, 2, 64)) * 40.0 * 1024.0) / 1024.0
    part = np.clip(part, -1000.0, 1000.0)
    gam = f32(r.uniform(0.5, 1.5, 64) * np.where(np.arange(64) % 5 == 2, -1.0, 1.0))
    return dict(partials=f32(part), gamma=gam, save_mean=f32(r.uniform(-2.0, 2.0, 64)), save_invstd=f32(r.uniform(0.3, 3.0, 64)),
                dgamma0=f32(r.standard_normal(64) * 30.0), dbeta0=f32(r.standard_normal(64) * 30.0), count=float(nparts * 192))


def bwd_ref(inp, accumulate, eval_mode):
    """float64 {A, C, B, sxh, s1, dgamma, dbeta} (dgamma, dbeta with the previous value where accumulate)"""
    s = sum_exact(inp["partials"])[0]
    mu, inv, ga, n = f64(inp["save_mean"]), f64(inp["save_invstd"]), f64(inp["gamma"]), inp["count"]
    sxh = (s[1] - mu * s[0]) * inv
    A = ga * inv
    C = np.zeros(64) if eval_mode else -ga * inv * inv * sxh / n
    Bv = np.zeros(64) if eval_mode else -(A * s[0] + C * mu * n) / n
    dg = sxh + (f64(inp["dgamma0"]) if accumulate else 0.0)
    db = s[0] + (f64(inp["dbeta0"]) if accumulate else 0.0)
    return dict(A=A, C=C, B=Bv, sxh=sxh, s1=s[0], dgamma=dg, dbeta=db)


def bwd_bound(ref, name, accumulate):
    if name in ("dgamma", "dbeta") and accumulate:
        return ulp32(ref["sxh" if name == "dgamma" else "s1"]) + ulp32(ref[name]) + TINY
    return ulp32(ref[name]) + TINY


def bwd_restated(inp, accumulate, eval_mode, defect=None):
    """{A, C, Bhi, Blo, dgamma, dbeta} float32 by the kernel's formula.  defect: "no_blo" hands B over as one word, "no_accumulate"
    overwrites dgamma / dbeta"""
    s = sum_exact(inp["partials"])[0]
    mu, inv, ga, n = f64(inp["save_mean"]), f64(inp["save_invstd"]), f64(inp["gamma"]), inp["count"]
    sxh = (s[1] - mu * s[0]) * inv
    Af = f32(ga * inv)
    Cf = np.zeros(64, dtype=np.float32) if eval_mode else f32(-ga * inv * inv * sxh / n)
    Bd = np.zeros(64) if eval_mode else -(f64(Af) * s[0] + f64(Cf) * (mu * n)) / n
    Bh = f32(Bd)
    Bl = np.zeros(64, dtype=np.float32) if defect == "no_blo" else f32(Bd - f64(Bh))
    acc = accumulate and defect != "no_accumulate"
    dg = inp["dgamma0"] + f32(sxh) if acc else f32(sxh)
    db = inp["dbeta0"] + f32(s[0]) if acc else f32(s[0])
    return dict(A=Af, C=Cf, Bhi=Bh, Blo=Bl, dgamma=dg, dbeta=db)


def zero_sum(inp, A, C, Bhi, Blo):
    """(|A s1 + (Bhi + Blo) count + C mu count|, the sum of the three magnitudes) per channel, in float64, from the kernel's words"""
    s1 = sum_exact(inp["partials"])[0][0]
    mu, n = f64(inp["save_mean"]), inp["count"]
    t = (f64(A) * s1, (f64(Bhi) + f64(Blo)) * n, f64(C) * mu * n)
    return np.abs(t[0] + t[1] + t[2]), np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2])


# the gradient scale of wm_bn_bwd_finalize: big = max |A| max dzmax (one float32 product), gs the power of two with big gs in
# (256, 512].  gscale_inputs makes max |A| exactly 1 (channel 0: gamma 2, invstd 0.5; every other |A| is smaller), so big = max dzmax.
BWD_NMAX = (1, 64, 1025)


def gscale_bwd_inputs(nparts=16):
    inp = bwd_inputs(nparts, seed=9)
    inp["gamma"] = f32(np.clip(inp["gamma"], -1.0, 1.0))
    inp["save_invstd"] = f32(np.clip(inp["save_invstd"], 0.3, 0.9))
    inp["gamma"][0], inp["save_invstd"][0] = 2.0, 0.5
    assert float(np.abs(f64(inp["gamma"]) * f64(inp["save_invstd"])).max()) == 1.0
    return inp


def dzmax_vector(m, nmax, where):
    """nmax maxima whose largest is m, at the first or the last entry; the others random below m / 2"""
    v = f32(rng(nmax).uniform(0.0, 0.5, nmax) * (m if np.isfinite(m) else 1.0))
    v[0 if where == "first" else nmax - 1] = m
    return v


# ------------------------------------------------------------------------ F. wm_gscale_absmax, wm_gscale_from_max, wm_absmax_rows
# The scale of a maximum m (finite, > 0) at target L is the one power of two gs with m gs in (2^(L-1), 2^L]: scale_exact, from the
# exponent of m.  Nothing is rounded: gs, 1 / gs and m gs are exact float32 numbers, so the three properties are asserted as
# equalities / strict inequalities.  scale_log2f restates what the kernels computed before (exp2f(floorf(L - log2f(m)))) in numpy's
# float32, for the CPU comparison of the two formulas.  All-zero, inf and NaN maxima give {1, 1}.  The kernels clamp gs to
# [1e-30, 1e30], ends that are no powers of two; there only the clamp itself and gs (1 / gs) within an ulp of 1 are promised.
GS_K = (-20, 0, 5, 12, 20)
GS_L = (9, 12)
GS_N = (4, 8188, 8192, 8196, 4 * (2048 * 1024) + 4)       # the last: the grid at its cap of 1024 workgroups and a ragged tail
GS_CLAMP = (1e-36, 3e37)
FROM_MAX_N = (1, 255, 256, 257)
ROWS_CASES = [(1, 4), (3, 8192), (3, 4 * (2048 * 64) + 4), (65535, 4)]      # (rows, row_len)


def gs_maxima():
    """2^k, the float32 above, the float32 below and the eighth float32 above (2^k (1 + 2^-20)), for k in GS_K"""
    out = []
    for k in GS_K:
        m = F32(2.0 ** k)
        out += [m, np.nextafter(m, F32(np.inf)), np.nextafter(m, F32(0)), F32(2.0 ** k * (1.0 + 2.0 ** -20))]
    return out


def scale_exact(m, L):
    """the power of two gs with m gs in (2^(L-1), 2^L] (L integral), as a Python float; 1.0 for 0, inf and NaN"""
    m = float(m)
    if not (m > 0.0 and m < 3.0e38):
        return 1.0
    f, e = math.frexp(m)                        # m = f 2^e, f in [0.5, 1)
    k = int(L) - e + (1 if f == 0.5 else 0)
    return min(max(math.ldexp(1.0, k), float(F32(1e-30))), float(F32(1e30)))


def scale_frexp(m, L, clamp=True):
    """the kernels' formula of today on float32 arrays: 2^(floor(L) - e + (f <= 2^(frac(L) - 1))), clamped"""
    m = f32(m)
    f, e = np.frexp(m)
    Li = np.floor(F32(L))
    fr = F32(L) - Li
    thr = F32(0.5) if fr == 0 else np.exp2(fr - F32(1.0), dtype=np.float32)
    with np.errstate(over="ignore", under="ignore"):
        gs = np.ldexp(F32(1.0), (Li.astype(np.int64) - e + (f <= thr)).astype(np.int32)).astype(np.float32)
    gs = np.where((m > 0) & (m < F32(3.0e38)), gs, F32(1.0))
    return np.minimum(np.maximum(gs, F32(1e-30)), F32(1e30)) if clamp else gs


def scale_log2f(m, L, binade_off=0, clamp=True):
    """the earlier formula, exp2f(floorf(L - log2f(m))), in numpy's float32, clamped; binade_off plants a scale that many binades off"""
    m = f32(m)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        gs = np.exp2(np.floor(F32(L) - np.log2(m, dtype=np.float32)) + F32(binade_off), dtype=np.float32)
    gs = np.where((m > 0) & (m < F32(3.0e38)), gs, F32(1.0))
    return np.minimum(np.maximum(gs, F32(1e-30)), F32(1e30)) if clamp else gs


def scale_log2f_div(m, clamp=True):
    """wm_bn_bwd_finalize's earlier formula, exp2f(floorf(log2f(512.f / big))), in numpy's float32"""
    m = f32(m)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        gs = np.exp2(np.floor(np.log2(F32(512.0) / m, dtype=np.float32)), dtype=np.float32)
    gs = np.where((m > 0) & (m < F32(3.0e38)), gs, F32(1.0))
    return np.minimum(np.maximum(gs, F32(1e-30)), F32(1e30)) if clamp else gs


def in_interval(m, gs, L):
    """m gs in (2^(L-1), 2^L], in float64 (the product of two float32 numbers is exact there)"""
    v = f64(m) * f64(gs)
    return (v > 2.0 ** (L - 1)) & (v <= 2.0 ** L)


def is_pow2(gs):
    f, _ = np.frexp(f64(gs))
    return f == 0.5


def absmax_input(n, m, where, seed=0):
    """n float32 in (-|m| / 2, |m| / 2) with m itself at the first or the last element; m may be negative, inf or NaN"""
    a = abs(float(m)) if np.isfinite(m) else 1.0
    x = f32(rng(600 + seed).uniform(-0.5, 0.5, n) * a)
    x[0 if where == "first" else n - 1] = m
    return x


# ---------------------------------------------------------------------------------- G. the producer chain: a whole ResBlock in training
# The statistics wm_bn_finalize is given come from the convolution kernels' epilogues, which sum x and x^2 in float32 per tile.  How far
# off-centre may the activations be before that one-pass variance costs accuracy?  One awm.ResBlock(64) in training mode against
# oracle.wm_oracle.resblock in float64 (it follows its input's dtype), with conv1's bias set so that the BN1 input has |mean| / std of
# about 0, 3 and 30 in every channel.  The rule is max(8 * e32, floor): floors 1e-5 for the output and the new running statistics, 2e-4
# for the gradients (a tenth of test_gpu_parity.py's tolerances).  For the quantities of BN1 itself -- its new running statistics and the
# gradients of its gamma and beta -- the floor is multiplied by 1 + mean^2 / var, the condition number of E[x^2] - E[x]^2: that much of
# float32's round-off in the two sums is the price of the one-pass formula and is not charged.  Everything else (the output, dx, the
# convolutions' weight gradients, BN2's quantities) keeps the plain floor, so an error of BN1's variance that reaches them shows.
# The convolution biases stand in front of a batch-statistics BatchNorm: their true gradient is zero and is not compared.
CHAIN_SHAPES = ((1, 64), (3, 132))
CHAIN_RATIOS = (0, 3, 30)
CHAIN_NAMES = ("out", "dx", "block.0.weight", "block.1.weight", "block.1.bias", "block.3.weight", "block.4.weight", "block.4.bias",
               "block.1.running_mean", "block.1.running_var", "block.4.running_mean", "block.4.running_var")
CHAIN_NBT = 3


def chain_inputs(ratio, B, T):
    """(state dict of a ResBlock(64), x [B, 64, T] post-ReLU-like, upstream gradient), float32"""
    g = torch.Generator().manual_seed(2000 + 10 * B + T)
    sd = {}
    for k in ("block.0.", "block.3."):
        sd[k + "weight"] = torch.randn(64, 64, 3, generator=g) * 0.08
        sd[k + "bias"] = torch.randn(64, generator=g) * 0.05
    for k in ("block.1.", "block.4."):
        sd[k + "weight"] = 0.8 + 0.4 * torch.rand(64, generator=g)
        sd[k + "bias"] = 0.05 * torch.randn(64, generator=g)
        sd[k + "running_mean"] = 0.05 * torch.randn(64, generator=g)
        sd[k + "running_var"] = 0.6 + 0.8 * torch.rand(64, generator=g)
        sd[k + "num_batches_tracked"] = torch.tensor(CHAIN_NBT)
    x = torch.randn(B, 64, T, generator=g).abs() * 0.7
    up = torch.randn(B, 64, T, generator=g)
    y = F.conv1d(x.double(), sd["block.0.weight"].double(), None, padding=1)
    sign = torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0).double()
    sd["block.0.bias"] = (ratio * y.std(dim=(0, 2), unbiased=False) * sign - y.mean(dim=(0, 2))).float()
    return sd, x, up


def chain_offcentre(ratio, B, T):
    """|mean| / std of the BN1 input per channel, in float64"""
    sd, x, _ = chain_inputs(ratio, B, T)
    y = F.conv1d(x.double(), sd["block.0.weight"].double(), sd["block.0.bias"].double(), padding=1)
    return (y.mean(dim=(0, 2)).abs() / y.std(dim=(0, 2), unbiased=False)).numpy()


def _chain_run(ratio, B, T, dtype):
    sd, x, up = chain_inputs(ratio, B, T)
    sdr = {k: (v.to(dtype).clone().requires_grad_() if v.is_floating_point() and "running" not in k else
               (v.to(dtype) if v.is_floating_point() else v.clone())) for k, v in sd.items()}
    xr = x.to(dtype).clone().requires_grad_()
    new = {}
    out = O.resblock(sdr, "", xr, True, new)
    out.backward(up.to(dtype))
    res = dict(out=out.detach(), dx=xr.grad)
    for k in CHAIN_NAMES[2:]:
        res[k] = new[k] if "running" in k else sdr[k].grad
    assert int(new["block.1.num_batches_tracked"]) == CHAIN_NBT + 1
    return res


@functools.lru_cache(maxsize=None)
def chain_ref(ratio, B, T):
    """(float64 reference, float32 reference): dicts over CHAIN_NAMES.  Computed once per case and shared; nobody writes to them."""
    return _chain_run(ratio, B, T, torch.float64), _chain_run(ratio, B, T, torch.float32)


def chain_floor(name, ratio):
    floor = 2e-4 if name == "dx" or name.endswith(("weight", "bias")) else 1e-5
    return floor * (1.0 + ratio * ratio) if name.startswith("block.1.") else floor
