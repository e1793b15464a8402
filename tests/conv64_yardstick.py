"""The float64 yardsticks of the 64-to-64 convolution launches (csrc/conv64_fwd.hip, conv64_dwgrad.hip, conv64_wgrad.hip, conv64_k7.hip,
conv64_eval.hip, conv64_fp32.hip), one reference per launch contract as include/wm_hip.h words it, with the input builders, the case
tables and the element-wise bounds, for tests/test_gpu_conv64_launches.py (GPU) and tests/test_conv64_yardstick_cpu.py (the references
against torch's float64 convolutions and autograd, a numpy restatement of each arithmetic meeting its bound in two accumulation orders,
and the same restatements with a defect planted missing it, without a GPU).  `import conv64_yardstick as Y`.  Numpy alone.

A launch is   y = epi(conv(pro(x)))   with side outputs.  Everything is written on the GEMM image W[tap][out][in] of the weight
(w_image: the four pack modes), so that one formula serves Conv1d k3 and ConvTranspose1d k7, forward and data gradient:
    acc[b, o, t] = sum_tap sum_in W[tap, o, in] pro(x)[b, in, t + tap - KW // 2]      (zero outside [0, T))
and the weight gradient is the same image on the other side:  dwimg[tap, o, in] = sum_{b, t} g'[b, o, t] x'[b, in, t + tap - KW // 2].

Bounds.  Derived per element from what the kernels document, none from a kernel's output.  With S the same convolution on absolute
values (sum |W| |pro(x)|) and n = 64 KW the accumulation length (B T for a weight gradient):
    native fp32 MFMA      gamma(n) S in any order.  Tightened by what the code fixes about the order: a matrix instruction sums MFMA_K
                          products (2 for v_mfma_f32_32x32x2_f32, 16 for the bf16 and f16 ones) and adds them to a float32 accumulator,
                          and the instructions of one output are chained, so a product passes through at most gamma(MFMA_K) inside its
                          instruction and chain(n) = pieces n / MFMA_K + 4 roundings of the accumulator:
                          (gamma(MFMA_K) + gamma(chain)) S, below gamma(pieces n) S from n = 16 on.  The same in the two lines below.
    bf16x6                three bf16 pieces (round to nearest, 8 bits each) hold a float32 exactly; of the nine piece products the kernels
                          keep the six of weight >= 2^-16 and drop (1,2), (2,1) and (2,2): 2 * 2^-24 + 2^-32 of |a b|, with 2^-7 of slack
                          for the pieces' own rounding (a piece is at most 2^-8 (1 + 2^-8) of the one above).  Then the accumulation of 6 n products.
    f16 two-piece split   hi = f16(a), lo = f16(a - hi): a is held to 2^-22 relative (11 + 11 bits), so the three kept products hi hi,
                          hi lo, lo hi carry 2 * 2^-22, and the dropped lo lo another 2^-22: 3 * 2^-22 (1 + 2^-10) S.  Below f16's normal
                          range lo is rounded to the subnormal spacing 2^-24: an ABSOLUTE 2^-25 per operand in the scaled domain, i.e.
                          2^-25 / gs per activation (gs = 1 where it is split unscaled) times sum |W|, and 2^-25 / ws per weight times
                          sum |pro(x)|.  ws, gs: the powers of two the pack kernels and the scale kernels define (weight_scale,
                          grad_scale below), exact factors.  Then the accumulation of 3 n products.
Prologue: its k roundings (fmaf chains: 1 for relu(x a + b) and x + v, 3 for the BatchNorm backward, 2 for the tail) are k U of the sum
of its terms' magnitudes P, carried through |W|.  Epilogue: every addition or product after the accumulator is one more U of the
magnitudes it combines; ELU (elu1: a 6th-order series above -0.35, __expf - 1 below) is documented to 4e-7 of the value, to which the
absolute 2^-21 of __expf's result near 1 is added.  stats, dw and dbias are sums over B T: the element bounds summed, plus
gamma(B T) of the summed magnitudes (any order), plus the final roundings.  max |y| is within the largest element bound.

Thresholds.  The builders keep every thresholded quantity away from its threshold: e1 ea + eb of EPI_RELUMASK is pushed to
|.| >= MARGIN = 1e-3 and the tail prologue's argument likewise, so no sample is ever left out: excluded_share() is 0 and asserted.

Restated on the CPU (tests/test_conv64_yardstick_cpu.py), worst |restatement - float64| / bound over the case inputs, two orders:
    native fp32 0.044    bf16x6 0.040    f16 split 0.040    (gamma is a worst-case bound: the round-off of random data grows as the
    root of the chain, not as the chain.  Since a faithful restatement uses less than a tenth, the bounds are re-checked from the other
    side: one product term off by 2^-12 of its size misses each of them, and so does every defect of the planted table.)

Measured on 1 x MI355X, the largest |kernel - float64| / bound of any compared element, per entry point (tests/test_gpu_conv64_launches.py
prints every figure):

    wm_conv64_bf          bf16x6: y 0.08, stats 0.02;  f16 split: y 0.98 (the bias addition's half ulp where the weights are 2^-20), stats 0.01
    wm_conv64             y 0.07, stats 0.01
    wm_wgrad64            dw 0.95 (T = 4 with accumulate: two roundings of one value), dbias 0.22
    wm_conv64_bf7         bf16x6 0.03;  f16 split 0.16
    wm_wgrad64_bf7        dw 0.91 (bf16x6), 0.94 (f16 split; gradient x 1e-9, activations x 1e-2: the floor term), dbias 0.22
    wm_wgrad64_bf         dw 0.56, dbias 0.21
    wm_dwgrad64_bf        bf16x6: y 0.05, stats 0.002, dw 0.10, dbias 0.02;  f16 split: y 0.21, stats 0.007, dw 0.96 (gradient x 1e-9,
                          activations x 1e-2: the floor term), dbias 0.02;  dzmax: exact
    wm_resblock_eval_bf   0.003
    wm_pack_w64_h*        hi + lo 0.94 of 2^-22 |v| + 2^-25;  {ws, 1 / ws} bit for bit

Findings.  (1) Fixed with this file: the native wm_conv64 ignored the low word pb[64 + c] of the BatchNorm-backward offset (5e-2 off
with a low word a tenth of the high one; 2^-24 of it in training, below what the composed tests see).  (2) Measured, kept as strict
expected failures of the project's bar of 1e-6 of max |ref| alone, with every element-wise bound met: activations of 1e-2 on the f16
split (wm_conv64_bf arith 1: 1.6e-6; dw of wm_dwgrad64_bf and wm_wgrad64_bf7 arith 1: 1.07e-6 to 1.41e-6), and seven taps at the shapes with the most
samples (native fp32 1.01e-6 to 1.29e-6, bf16x6 1.04e-6).
"""
import numpy as np

from yardstick_common import U, gamma

F32 = np.float32
KNUMCU = 256
MARGIN = 1e-3
STATS_FLOATS, DZMAX_FLOATS = 256 * 128, 256
PARTIAL_SLABS = 256
ARITHS = ("fp32", "bf", "h")
DROP_BF = (2 * 2.0 ** -24 + 2.0 ** -32) * (1 + 2.0 ** -7)
DROP_H = 3 * 2.0 ** -22 * (1 + 2.0 ** -10)
FLOOR_H = 2.0 ** -25
PRO_NONE, PRO_BNRELU, PRO_ADDVEC, PRO_BNBWD, PRO_TAIL = 0, 1, 2, 3, 4
EPI_BIAS, EPI_RELUMASK, EPI_ADD, EPI_NONE, EPI_BNADDRELU, EPI_BIASELU, EPI_BIASADDELU, EPI_MULDELU, EPI_ADDSTATS = range(9)
PRO_ROUNDINGS = {PRO_NONE: 0, PRO_BNRELU: 1, PRO_ADDVEC: 1, PRO_BNBWD: 3, PRO_TAIL: 2}


def rng(seed):
    return np.random.default_rng(seed)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------- the mask word layout, stated once
def encode_mask(pos):
    """bool [B, 64, T] -> uint32 [B * 64, ceil(T / 32)]: wm_bn_add_relu_mask's layout, bit t % 32 of word t / 32, the bits past T clear"""
    B, C, T = pos.shape
    nw = (T + 31) // 32
    padded = np.zeros((B * C, nw * 32), dtype=np.uint64)
    padded[:, :T] = pos.reshape(B * C, T)
    return (padded.reshape(B * C, nw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def decode_mask(words, B, T):
    """uint32 [B * 64, nw] -> bool [B, 64, T]"""
    b = (words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return b.reshape(words.shape[0], -1)[:, :T].astype(bool).reshape(B, 64, T)


# ------------------------------------------------------------------------------------------------------------- weights and scales
def w_image(w, mode):
    """the GEMM image W[tap][out][in] (float64) of a weight: mode 0 Conv1d [out][in][KW] forward | 1 its data gradient (channels
    transposed, taps flipped) | 2 ConvTranspose1d [in][out][KW] forward (the same transposition and flip) | 3 its data gradient"""
    w = f64(w)
    if mode in (0, 3):
        return np.ascontiguousarray(w.transpose(2, 0, 1))
    return np.ascontiguousarray(w[:, :, ::-1].transpose(2, 1, 0))


def dw_from_image(img, layout):
    """dwimg[tap][o][i] -> layout 0: Conv1d's dw[o][i][tap] | 1: ConvTranspose1d's dw[i][o][KW - 1 - tap]"""
    return img.transpose(1, 2, 0) if layout == 0 else img[::-1].transpose(2, 1, 0)


def _pow2_floor_log2(v):
    """2^floor(log2(v)) for a positive float, exactly"""
    f, e = np.frexp(v)
    return float(np.ldexp(1.0, int(e) - 1))


def weight_scale(w, row_scale=None):
    """{ws, 1 / ws} of pack_w64_h_kernel / pack_w64_h7_kernel: ws = 2^floor(log2(1023 / m)), m = max |w (row_scale[out])| in float32;
    1 for m = 0 or m >= 3e38; clamped to [1e-30, 1e30] (ends that are no powers of two).  The quotient 1023 / m is the float32 one."""
    v = f32(w) if row_scale is None else f32(w) * f32(row_scale)[:, None, None]
    m = F32(np.abs(v).max())
    ws = F32(1.0)
    if m > 0 and m < F32(3.0e38):
        with np.errstate(over="ignore"):
            q = F32(1023.0) / m
        ws = F32(_pow2_floor_log2(float(q))) if np.isfinite(q) else F32(np.inf)
    ws = min(max(ws, F32(1e-30)), F32(1e30))
    return F32(ws), F32(1.0) / F32(ws)


def grad_scale(m, L):
    """{gs, 1 / gs} of wm_gscale_absmax / wm_gscale_from_max / wm_bn_bwd_finalize for the maximum m: the power of two with m gs in
    (2^(L-1), 2^L]; 1 for 0, inf and NaN; clamped to [1e-30, 1e30]"""
    m = float(m)
    if not (m > 0.0 and m < 3.0e38):
        return F32(1.0), F32(1.0)
    f, e = np.frexp(m)
    gs = F32(min(max(float(np.ldexp(1.0, int(L) - int(e) + (1 if f == 0.5 else 0))), float(F32(1e-30))), float(F32(1e30))))
    return gs, F32(1.0) / gs


def decode_h_image(img_u16, kw):
    """the bytes of a wm_pack_w64_h* image -> (hi + lo as float64 [kw][64][64], ws, 1 / ws)"""
    n = kw * 4096
    h = img_u16[:2 * n].view(np.float16).astype(np.float64)
    tail = img_u16[2 * n:2 * n + 4].view(np.float32)
    return (h[:n] + h[n:]).reshape(kw, 64, 64), tail[0], tail[1]


# ---------------------------------------------------------------------------------------------------------------------- prologues
def pro_ref(pro, x, x2=None, pa=None, pb=None, pc=None):
    """(pro(x), P) in float64: P = the sum of the magnitudes of the prologue's terms (its roundings are PRO_ROUNDINGS[pro] U P).
    0 x | 1 relu(x pa[c] + pb[c]) | 2 x + pa[b, c] | 3 pa[c] x + pb[0, c] + pb[1, c] + pc[c] x2 | 4 relu(x + x2 pa[c] + pb[c])"""
    x = f64(x)
    ch = (lambda v: f64(v)[None, :, None])
    if pro == PRO_NONE:
        return x, np.abs(x)
    if pro == PRO_BNRELU:
        return np.maximum(x * ch(pa) + ch(pb), 0.0), np.abs(x * ch(pa)) + np.abs(ch(pb))
    if pro == PRO_ADDVEC:
        v = f64(pa).reshape(x.shape[0], 64)[:, :, None]
        return x + v, np.abs(x) + np.abs(v)
    if pro == PRO_BNBWD:
        pb = f64(pb).reshape(2, 64)
        terms = (ch(pa) * x, ch(pb[0]) + 0 * x, ch(pb[1]) + 0 * x, ch(pc) * f64(x2))
        return sum(terms), sum(np.abs(t) for t in terms)
    if pro == PRO_TAIL:
        t = f64(x2) * ch(pa)
        return np.maximum(x + t + ch(pb), 0.0), np.abs(x) + np.abs(t) + np.abs(ch(pb))
    raise ValueError(pro)


def pro_args(pro, d):
    """the prologue's operands among a builder's arrays, as a launch is handed them: dict(x2, pa, pb, pc)"""
    if pro == PRO_BNRELU:
        return dict(pa=d["pa"], pb=d["pb"][0])
    if pro == PRO_ADDVEC:
        return dict(pa=d["vec"])
    if pro == PRO_BNBWD:
        return dict(x2=d["x2"], pa=d["pa"], pb=d["pb"], pc=d["pc"])
    if pro == PRO_TAIL:
        return dict(x2=d["x2"], pa=d["pa"], pb=d["pb"][0])
    return {}


def conv_img(W, xin):
    """acc[b, o, t] = sum_tap sum_in W[tap, o, in] xin[b, in, t + tap - KW // 2], zero padding; float64"""
    kw, T = W.shape[0], xin.shape[2]
    xp = np.pad(f64(xin), ((0, 0), (0, 0), (kw // 2, kw // 2)))
    return sum(np.matmul(W[k], xp[:, :, k:k + T]) for k in range(kw))


def wgrad_img(g, xin, kw):
    """dwimg[tap, o, i] = sum_{b, t} g[b, o, t] xin[b, i, t + tap - KW // 2]; float64"""
    T = xin.shape[2]
    xp = np.pad(f64(xin), ((0, 0), (0, 0), (kw // 2, kw // 2)))
    G = np.ascontiguousarray(f64(g).transpose(1, 0, 2)).reshape(64, -1)
    return np.stack([G @ np.ascontiguousarray(xp[:, :, k:k + T].transpose(0, 2, 1)).reshape(-1, xp.shape[1]) for k in range(kw)])


MFMA_K = {"fp32": 2, "bf": 16, "h": 16}          # products one matrix instruction sums: 32x32x2 f32, 32x32x16 bf16, 32x32x16 f16
PIECE_PRODUCTS = {"fp32": 1, "bf": 6, "h": 3}


def chain(arith, n):
    """the most float32 additions a product of an n-term sum passes through: the instructions chained on one accumulator, PIECE_PRODUCTS
    for every MFMA_K terms, and 4 more for whatever joins partial accumulators (halves of a tile, the waves of a workgroup)"""
    return PIECE_PRODUCTS[arith] * -(-n // MFMA_K[arith]) + 4


def arith_const(arith, n):
    """the relative constant of an accumulation of n products in the arithmetic (module text)"""
    return {"fp32": 0.0, "bf": DROP_BF, "h": DROP_H}[arith] + gamma(MFMA_K[arith]) + gamma(chain(arith, n))


def elu(v):
    return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))


ELU_REL, ELU_ABS = 4e-7, 2.0 ** -21


# -------------------------------------------------------------------------------------------------------- one forward / dgrad launch
def conv_ref(inp, kw, mode, pro, epi, arith="fp32", ws=1.0, gs=1.0, stats=False, gmask=None, defect=None):
    """The launch y = epi(conv(pro(x))) in float64 with its bound.  inp: dict of float32 arrays (conv_inputs).  Returns dict:
    y, bound (element-wise), stats [2, 64] and stats_bound (where the epilogue has sums), ymax (max |y|), ymax_bound.
    epi 0 + bias | 1 keep where e1 ea + eb > 0, sums (y, y e1) | 2 + e1 | 3 none | 4 relu(e1 + (acc + bias) ea + eb) | 5 elu(acc + bias) |
    6 elu(acc + bias + e1) | 7 acc ELU'(e1), e1 = an ELU output | 8 (acc + e1 [gmask]) [pmask], sums (y, y ea[b, c, t]).
    epi 0 with stats: sums (y, y^2).  gmask: None | "x" (x is kept where inp["gmask"] is set, before the prologue: the first form of
    wm_dwgrad64_bf) | "e1" (the addend of epi 2 likewise: its second form; epi 8 always masks its addend).  inp["gmask"], inp["pmask"]:
    bool arrays, the decoded bits."""
    W = w_image(inp["w"], mode)
    x = np.where(inp["gmask"], f64(inp["x"]), 0.0) if gmask == "x" else inp["x"]
    xin, P = pro_ref(pro, x, **pro_args(pro, inp))
    acc, Wabs = conv_img(W, xin), np.abs(W)
    S = conv_img(Wabs, np.abs(xin))
    n = 64 * kw
    bound = arith_const(arith, n) * S + PRO_ROUNDINGS[pro] * U * conv_img(Wabs, P)
    if arith == "h":
        wsum = conv_img(Wabs, np.ones_like(xin))
        xsum = conv_img(np.ones_like(W), np.abs(xin))
        bound = bound + FLOOR_H / float(gs) * wsum + FLOOR_H / float(ws) * xsum
    ch = (lambda v: f64(v)[None, :, None])
    bias = ch(inp["bias"]) if inp.get("bias") is not None else 0.0
    e1 = f64(inp["e1"]) if inp.get("e1") is not None else None
    out = {}
    if epi == EPI_BIAS:
        y = acc + bias
        bound = bound + U * (np.abs(acc) + np.abs(bias))
        if stats:
            sums, sb = (y, y * y), (bound, 2 * np.abs(y) * bound + bound * bound + U * y * y)
    elif epi == EPI_RELUMASK:
        keep = e1 * ch(inp["ea"]) + ch(inp["eb"]) > 0
        y, bound = np.where(keep, acc, 0.0), np.where(keep, bound, 0.0)
        sums, sb = (y, y * e1), (bound, bound * np.abs(e1) + U * np.abs(y * e1))
    elif epi == EPI_ADD:
        add = np.where(inp["gmask"], e1, 0.0) if gmask == "e1" else e1
        y = acc + add
        bound = bound + U * (np.abs(acc) + np.abs(add))
    elif epi == EPI_NONE:
        y = acc
    elif epi == EPI_BNADDRELU:
        t = (acc + bias) * ch(inp["ea"])
        y = np.maximum(e1 + t + ch(inp["eb"]), 0.0)
        bound = bound * np.abs(ch(inp["ea"])) + U * (np.abs(acc) + np.abs(bias)) * np.abs(ch(inp["ea"])) + \
            2 * U * (np.abs(t) + np.abs(ch(inp["eb"])) + np.abs(e1))
    elif epi in (EPI_BIASELU, EPI_BIASADDELU):
        v = acc + bias + (e1 if epi == EPI_BIASADDELU else 0.0)
        y = elu(v)
        bound = bound + 2 * U * (np.abs(acc) + np.abs(bias) + (np.abs(e1) if epi == EPI_BIASADDELU else 0.0)) + ELU_REL * np.abs(y) + ELU_ABS
    elif epi == EPI_MULDELU:
        d = np.where(e1 > 0, 1.0, e1 + 1.0)
        y = acc * d
        bound = bound * np.abs(d) + 2 * U * np.abs(y)
    elif epi == EPI_ADDSTATS:
        add = np.where(inp["gmask"], e1, 0.0)
        y = np.where(inp["pmask"], acc + add, 0.0)
        bound = np.where(inp["pmask"], bound + U * (np.abs(acc) + np.abs(add)), 0.0)
        py2 = f64(inp["py2"])
        sums, sb = (y, y * py2), (bound, bound * np.abs(py2) + U * np.abs(y * py2))
    else:
        raise ValueError(epi)
    BT = y.shape[0] * y.shape[2]
    if defect == "ragged4":
        y = y.copy()
        y[:, :, -4:] = 0.0
    out.update(y=y, bound=bound, S=S, ymax=float(np.abs(y).max()), ymax_bound=float(bound.max()))
    if stats or epi in (EPI_RELUMASK, EPI_ADDSTATS):
        out["stats"] = np.stack([s.sum(axis=(0, 2)) for s in sums])
        out["stats_bound"] = np.stack([b.sum(axis=(0, 2)) + gamma(BT) * np.abs(s).sum(axis=(0, 2)) for s, b in zip(sums, sb)]) + 1e-300
    return out


def wgrad_ref(g, x, kw, layout, arith="fp32", gs=1.0, g_err=None, x_err=None, prev=None):
    """The weight-gradient launch on the already formed operands g' and x' (float64, from pro_ref): dict dw (in `layout`), dbias [64],
    and their bounds.  g_err / x_err: the element bounds of the operands' own roundings (k U P).  prev: (dw0, dbias0) float32 for
    accumulate.  The slabs are summed in double and rounded once (wgrad64_reduce_kernel): U of the result, and U more with accumulate.
    arith h: g is split under the scale gs, x unscaled."""
    B, _, T = g.shape
    BT = B * T
    img, Simg = wgrad_img(g, x, kw), wgrad_img(np.abs(g), np.abs(x), kw)
    bimg = arith_const(arith, BT) * Simg
    if g_err is not None:
        bimg = bimg + wgrad_img(g_err, np.abs(x), kw)
    if x_err is not None:
        bimg = bimg + wgrad_img(np.abs(g), x_err, kw)
    if arith == "h":
        bimg = bimg + FLOOR_H * wgrad_img(np.abs(g), np.ones_like(x), kw) + FLOOR_H / float(gs) * wgrad_img(np.ones_like(g), np.abs(x), kw)
    db = g.sum(axis=(0, 2))
    dbb = gamma(BT) * np.abs(g).sum(axis=(0, 2)) + (g_err.sum(axis=(0, 2)) if g_err is not None else 0.0)
    dw, dwb = dw_from_image(img, layout), dw_from_image(bimg, layout)
    dwb, dbb = dwb + U * np.abs(dw), dbb + U * np.abs(db)
    if prev is not None:
        dw, db = dw + f64(prev[0]), db + f64(prev[1])
        dwb, dbb = dwb + U * np.abs(dw), dbb + U * np.abs(db)
    return dict(dw=np.ascontiguousarray(dw), dw_bound=np.ascontiguousarray(dwb) + 1e-300, dbias=db, dbias_bound=dbb + 1e-300)


def resblock_eval_ref(x, w1, b1, sc1, sh1, w2, b2, sc2, sh2, arith):
    """y = relu(x + (conv2(relu((conv1(x) + b1) sc1 + sh1)) + b2) sc2 + sh2) in float64, and its bound: the first convolution's bound
    (weights w1 sc1[out]) through the second one's |weights|, the second one's own, and the epilogue's three roundings"""
    ch = (lambda v: f64(v)[None, :, None])
    x = f64(x)
    W1, W2 = w_image(f64(w1) * f64(sc1)[:, None, None], 0), w_image(f64(w2) * f64(sc2)[:, None, None], 0)
    o1 = (f64(b1) if b1 is not None else 0.0) * f64(sc1) + f64(sh1)
    o2 = (f64(b2) if b2 is not None else 0.0) * f64(sc2) + f64(sh2)
    a1 = conv_img(W1, x)
    c = arith_const(arith, 192)
    e1 = (c + U) * conv_img(np.abs(W1), np.abs(x)) + 3 * U * (np.abs(a1) + np.abs(ch(o1)))      # + the rounding of w sc in the image
    h = np.maximum(a1 + ch(o1), 0.0)
    a2 = conv_img(W2, h)
    e2 = (c + U) * conv_img(np.abs(W2), h) + conv_img(np.abs(W2), e1)
    if arith == "h":
        ws1, ws2 = weight_scale(w1, sc1)[0], weight_scale(w2, sc2)[0]
        e2 = e2 + FLOOR_H * conv_img(np.abs(W2), np.ones_like(x)) + FLOOR_H / float(ws2) * conv_img(np.ones_like(W2), h) + \
            conv_img(np.abs(W2), FLOOR_H * conv_img(np.abs(W1), np.ones_like(x)) + FLOOR_H / float(ws1) * conv_img(np.ones_like(W1), np.abs(x)))
    y = np.maximum(x + a2 + ch(o2), 0.0)
    return y, e2 + 3 * U * (np.abs(x) + np.abs(a2) + np.abs(ch(o2)))


# ------------------------------------------------------------------------------------------------------------------ input builders
def conv_inputs(B, T, kw=3, seed=0, wscale=0.08, xscale=1.0, e1scale=1.0, cscale=1.0, outlier=None):
    """every operand a launch may take, float32, from one seed: x, x2, e1, py2 [B, 64, T]; w ([out][in][kw], or [in][out][kw]: both
    are [64][64][kw]); pa, pc, bias, ea, eb [64]; pb [2][64] (hi and a lo word of a tenth of its size: the contract is their sum);
    vec [B, 64]; gmask, pmask bool [B, 64, T].  e1 is moved until |e1 ea + eb| >= MARGIN everywhere (x, pa, pb[0] likewise for the tail
    prologue's argument x + x2 pa + pb[0]); the largest |x|, 6 xscale, sits in the last quarter of the last row.  xw: one more frame (the
    weight gradient's operand where x is the gradient).  cscale multiplies pc (a gradient-sized constant where x is a gradient);
    outlier: |x| at (0, 3, 100 % T) in units of xscale (the element that sets a gradient scale, the bulk far below it)."""
    r = rng(9000 + 131 * B + T + 7 * kw + seed)
    d = dict(x=r.standard_normal((B, 64, T)) * xscale, x2=r.standard_normal((B, 64, T)), e1=r.standard_normal((B, 64, T)) * e1scale,
             py2=r.standard_normal((B, 64, T)), w=r.standard_normal((64, 64, kw)) * wscale,
             pa=r.uniform(0.5, 1.5, 64) * np.where(np.arange(64) % 4 == 1, -1.0, 1.0), pc=r.uniform(-0.5, 0.5, 64),
             bias=r.standard_normal(64) * 0.1, ea=r.uniform(0.5, 1.5, 64) * np.where(np.arange(64) % 5 == 2, -1.0, 1.0),
             eb=r.uniform(-0.5, 0.5, 64) * e1scale, vec=r.standard_normal((B, 64)))
    pbh = r.uniform(-0.5, 0.5, 64) * xscale
    d["pb"] = np.stack([pbh, 0.1 * pbh * r.uniform(0.5, 1.0, 64)])
    d = {k: f32(v) for k, v in d.items()}
    d["pc"] = f32(d["pc"] * F32(cscale))
    d["xw"] = f32(rng(77000 + 131 * B + T + seed).standard_normal((B, 64, T)) * e1scale)
    d["x"][B - 1, 63, T - 1] = 6.0 * xscale
    if outlier is not None:
        d["x"][0, 3, 100 % T] = outlier * xscale
    d["gmask"], d["pmask"] = r.random((B, 64, T)) < 0.55, r.random((B, 64, T)) < 0.55
    for _ in range(8):
        bad = ~margin_ok(d)
        if not bad.any():
            break
        d["e1"][bad] += F32(4 * MARGIN * e1scale + 4 * MARGIN)
    for _ in range(8):
        bad = ~tail_margin_ok(d)
        if not bad.any():
            break
        d["x"][bad] += F32(4 * MARGIN)
    return d


def margin_ok(d):
    return np.abs(f64(d["e1"]) * f64(d["ea"])[None, :, None] + f64(d["eb"])[None, :, None]) >= MARGIN


def tail_margin_ok(d):
    return np.abs(f64(d["x"]) + f64(d["x2"]) * f64(d["pa"])[None, :, None] + f64(d["pb"][0])[None, :, None]) >= MARGIN


def excluded_share(d):
    """the share of samples a comparison would have to leave out because a thresholded quantity is within MARGIN of its threshold"""
    return float(np.mean(~margin_ok(d) | ~tail_margin_ok(d)))


# ------------------------------------------------------------------------------------- the arithmetics restated (CPU test, defects)
def bf16_rn(a):
    """float32 -> the nearest bf16 (ties to even), as float32"""
    b = f32(a).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def split_bf(a):
    """split3_pair: three bf16 pieces, each the rounding of what the ones above leave"""
    a = f32(a)
    p0 = bf16_rn(a)
    p1 = bf16_rn(a - p0)
    return [p0, p1, bf16_rn(a - p0 - p1)]


def split_h(a):
    """the two-piece f16 split: hi = f16(a), lo = f16(a - hi)"""
    a = f32(a)
    with np.errstate(over="ignore"):
        hi = a.astype(np.float16).astype(np.float32)
        return [hi, (a - hi).astype(np.float16).astype(np.float32)]


KEPT = {"fp32": [(0, 0)], "bf": [(1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0)], "h": [(1, 0), (0, 1), (0, 0)]}


def pieces(arith, a):
    return {"fp32": lambda v: [f32(v)], "bf": split_bf, "h": split_h}[arith](a)


def mm_restated(arith, W, xin, order=0, ws=1.0, gs=1.0):
    """conv_img in the kernels' arithmetic: the operands in float32 (weights times ws, activations times gs and clamped to +-6e4 for h),
    split into pieces, exactly the kept piece products, MFMA_K input channels at a time summed exactly (one matrix instruction) and
    added to a float32 accumulator -- taps and channel blocks forwards (order 0) or backwards (order 1); the result times 1 / (ws gs)"""
    kw, T = W.shape[0], xin.shape[2]
    Wf, xf = f32(f32(W) * F32(ws)), f32(xin)
    if arith == "h":
        xf = np.clip(f32(xf * F32(gs)), F32(-6.0e4), F32(6.0e4))
    A = [f64(p) for p in pieces(arith, Wf)]
    Bp = [np.pad(f64(p), ((0, 0), (0, 0), (kw // 2, kw // 2))) for p in pieces(arith, xf)]
    acc = np.zeros((xin.shape[0], 64, T), dtype=np.float32)
    K = MFMA_K[arith]
    taps, blocks = list(range(kw)), list(range(0, 64, K))
    if order:
        taps, blocks = taps[::-1], blocks[::-1]
    for k in taps:
        for c in blocks:
            for i, j in KEPT[arith]:
                acc = f32(f64(acc) + np.matmul(A[i][k][:, c:c + K], Bp[j][:, c:c + K, k:k + T]))
    return f32(f64(acc) * (1.0 / (float(ws) * float(gs))))


def pro_restated(pro, x, x2=None, pa=None, pb=None, pc=None, defect=None):
    """pro_apply in float32 (a fused multiply-add: the product in double, one rounding)"""
    ch = (lambda v: f64(v)[None, :, None])
    x = f32(x)
    if pro == PRO_NONE:
        return x
    if pro == PRO_BNRELU:
        return np.maximum(f32(f64(x) * ch(pa) + ch(pb)), F32(0))
    if pro == PRO_ADDVEC:
        return x + f32(pa).reshape(x.shape[0], 64)[:, :, None]
    if pro == PRO_BNBWD:
        pb = f32(pb).reshape(2, 64)
        inner = f32(ch(pc) * f64(x2) + ch(pb[0]))
        v = f32(ch(pa) * f64(x) + f64(inner))
        return v if defect == "no_pb_lo" else v + pb[1][None, :, None]
    if pro == PRO_TAIL:
        return np.maximum(x + f32(f64(x2) * ch(pa) + ch(pb)), F32(0))
    raise ValueError(pro)


# -------------------------------------------------------------------------------------------------------------------- case tables
# shapes: the smallest at which each path still differs (module text of tests/test_gpu_conv64_launches.py)
SERIAL_SHAPES = ((1, 4), (1, 8), (2, 124), (3, 132), (2, 260), (129, 132))
PIPE_SHAPES = ((1, 128), (7, 128), (8, 128), (2, 384), (257, 128), (2, 16512))
COL64_SHAPES = ((1, 64), (7, 64), (2, 192), (257, 64), (2, 8256))
MID_PIPE, MID_COL64 = (2, 384), (2, 192)
BN_ROWS = ((0, 0, True), (0, 0, False), (1, 0, True), (1, 0, False), (3, 1, True), (3, 2, False), (3, 3, False))      # (pro, epi, stats)
ELU_ROWS = ((0, 2, False), (0, 3, False), (0, 5, False), (0, 6, False), (0, 7, False))
# wm_conv64_bf: (kernel, arith, pro, epi, stats, shapes)
CONV3_BF_CASES = [("serial", "bf", p, e, s, SERIAL_SHAPES) for p, e, s in BN_ROWS + ELU_ROWS] + \
    [("pipe", "bf", p, e, s, PIPE_SHAPES) for p, e, s in BN_ROWS + ((1, 4, False),)] + \
    [("pipe", "h", p, e, s, PIPE_SHAPES) for p, e, s in BN_ROWS[:4] + ((1, 4, False),)]
# wm_conv64 (native): (kw, pro, epi, stats)
CONV_NATIVE_CASES = [(3, p, e, s) for p, e, s in BN_ROWS] + [(7, 0, 0, False), (7, 2, 0, False), (7, 0, 3, False)]
# wm_wgrad64 (native): (kw, gpro, xpro, layout)
WGRAD_NATIVE_CASES = [(3, 3, 1, 0), (3, 3, 0, 0), (3, 3, 1, 1), (7, 0, 2, 1), (7, 0, 0, 1), (7, 0, 0, 0)]
# wm_conv64_bf7: (kernel, arith, pro, epi, gscale given)
CONV7_CASES = [(k, a, p, e, g) for k in ("ragged", "pipe") for a in ("bf", "h") for p, e in ((0, 0), (2, 0), (0, 3)) for g in (False, True)
               if (a == "h" and k == "pipe") or (a == "bf" and not g)]
WGRAD7_CASES = [(a, xp) for a in ("bf", "h") for xp in (0, 2)]
WGRAD3_BF_CASES = [(3, 1), (3, 0), (0, 0)]                 # (gpro, xpro); accumulate 0..3 inside
# wm_dwgrad64_bf: (xpro, epi, gmask, arith)
DWGRAD_CASES = [(x, e, m, a) for x, e in ((1, 1), (0, 2), (0, 8)) for m in (False, True) for a in ("bf", "h") if not (e == 8 and not m)]
# the scale axis of arith h, at one mid shape: weights, incoming gradient (one outlier 32 x the bulk), activations
H_WSCALES, H_GSCALES, H_XSCALES = (2.0 ** -20, 1.0, 2.0 ** 10), (1e-9, 1.0, 3e4), (1e-2, 30.0)

# every dispatcher branch of the six units that returns a launch, by the template instance it starts: the matrix the case tables must
# cover (tests/test_conv64_yardstick_cpu.py::test_cases_cover_the_launch_matrix)
MATRIX = {
    "wm_conv64_bf": [("serial", "bf") + r for r in BN_ROWS + ELU_ROWS] + [("pipe", "bf") + r for r in BN_ROWS + ((1, 4, False),)] +
                    [("pipe", "h") + r for r in BN_ROWS[:4] + ((1, 4, False),)],
    "wm_conv64": [(3,) + r for r in BN_ROWS] + [(7, 0, 0, False), (7, 2, 0, False), (7, 0, 3, False)],
    "wm_wgrad64": [(3, 3, 1), (3, 3, 0), (7, 0, 2), (7, 0, 0)],
    "wm_conv64_bf7": [(k, a, p, e) for k in ("ragged", "pipe") for a in ("bf", "h") for p, e in ((0, 0), (2, 0), (0, 3)) if not (a == "h" and k == "ragged")],
    "wm_wgrad64_bf7": [("bf", 0), ("bf", 2), ("h", 0), ("h", 2)],
    "wm_wgrad64_bf": [(3, 1, False), (3, 0, False), (0, 0, False), (3, 1, True), (3, 0, True)],      # (gpro, xpro, output-split build)
    "wm_dwgrad64_bf": [(x, e, m, a) for x, e in ((1, 1), (0, 2), (0, 8)) for m in (False, True) for a in ("bf", "h") if not (e == 8 and not m)],
    "wm_resblock_eval_bf": ["bf", "h"],
}


def covered():
    """what the case tables reach, in MATRIX's terms"""
    return {
        "wm_conv64_bf": [(k, a, p, e, s) for k, a, p, e, s, _ in CONV3_BF_CASES],
        "wm_conv64": list(CONV_NATIVE_CASES),
        "wm_wgrad64": [(kw, gp, xp) for kw, gp, xp, _ in WGRAD_NATIVE_CASES],
        "wm_conv64_bf7": [(k, a, p, e) for k, a, p, e, _ in CONV7_CASES],
        "wm_wgrad64_bf7": list(WGRAD7_CASES),
        "wm_wgrad64_bf": [(gp, xp, small) for gp, xp in WGRAD3_BF_CASES for small in (False, True) if not (small and gp == 0)],
        "wm_dwgrad64_bf": list(DWGRAD_CASES),
        "wm_resblock_eval_bf": ["bf", "h"],
    }
