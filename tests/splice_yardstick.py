"""Yardsticks for the splice attack and the localisation kernels, written from the definitions in include/wm_hip.h in integer / float64 numpy.
Nothing from the package: the Philox4x32-10 of tests/draw_yardstick.py, its own integer geometry, its own bit packing, its own BCE."""
import numpy as np

from draw_yardstick import key_of, philox4x32_10, splice_shift, splice_span

ORIGINAL, SILENCE, MOVED = 0, 1, 2


def spans(seed, draw, row, n, max_spans, p_span, len_lo, len_hi, p_original, p_silence):
    """[(start, L, kind, shift, active)] for span j = 0 .. max_spans - 1 of row `row` (= row0 + r)"""
    key = key_of(seed)
    t_span = float(np.float32(p_span))                                 # float32 arguments, compared in float64
    t_orig = float(np.float32(p_original))
    t_sil = t_orig + float(np.float32(p_silence))
    out = []
    for j in range(max_spans):
        o = [int(w) for w in philox4x32_10((*splice_span(j), row, draw), key)]
        o2 = [int(w) for w in philox4x32_10((*splice_shift(j), row, draw), key)]
        v = [w >> 9 for w in o]
        u = [(w + 0.5) * 2.0 ** -23 for w in v]
        L = len_lo + ((v[1] * (len_hi - len_lo + 1)) >> 23)
        start = (v[2] * (n - L + 1)) >> 23
        kind = ORIGINAL if u[3] < t_orig else (SILENCE if u[3] < t_sil else MOVED)
        if n == 1 and kind == MOVED:
            kind = ORIGINAL
        shift = 1 + (((o2[0] >> 9) * (n - 1)) >> 23)
        out.append((start, L, kind, shift, u[0] < t_span))
    return out


def splice(a, b, seed, draw, row0, **cut):
    """(y float32 (rows, n), labels bool (rows, n)): per sample, the LARGEST active j whose span holds it decides"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    rows, n = a.shape
    y, labels = np.empty_like(a), np.empty((rows, n), dtype=bool)
    t = np.arange(n)
    for r in range(rows):
        owner = np.full(n, -1)
        sp = spans(seed, draw, row0 + r, n, **cut)
        for j, (start, L, kind, shift, active) in enumerate(sp):
            if active:
                owner[(t >= start) & (t < start + L)] = j              # rising j: the largest stays
        labels[r] = owner < 0
        row = a[r].copy()
        for j, (start, L, kind, shift, active) in enumerate(sp):
            m = owner == j
            row[m] = b[r][t[m]] if kind == ORIGINAL else (np.float32(0.0) if kind == SILENCE else b[r][(t[m] + shift) % n])
        y[r] = row
    return y, labels


def pack(labels):
    """bool (rows, n) -> uint32 (rows, ceil(n / 32)); bit j of word w is sample 32 w + j; tail bits zero"""
    labels = np.asarray(labels, dtype=bool)
    rows, n = labels.shape
    W = (n + 31) // 32
    words = np.zeros((rows, W), dtype=np.uint64)
    for t in range(n):
        words[:, t // 32] |= labels[:, t].astype(np.uint64) << np.uint64(t % 32)
    return words.astype(np.uint32)


def unpack(words, n):
    words = np.asarray(words).view(np.uint32)
    return np.stack([(words[:, t // 32] >> np.uint32(t % 32)) & np.uint32(1) for t in range(n)], axis=1).astype(bool)


def bce64(x, y):
    """BCEWithLogits element-wise in float64: max(x, 0) - x y + log1p(exp(-|x|))"""
    return np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))


def masked_losses(logits, message, labels, B):
    """(loc, bce, N1, dloc/dlogits, dbce/dlogits) in float64.  logits (R, T, NO); labels bool (B, T); message (B,) ints"""
    x = np.asarray(logits, dtype=np.float64)
    R, T, NO = x.shape
    y = np.zeros((R, T))
    y[:B] = labels
    loc = bce64(x[:, :, 0], y).sum() / (R * T)
    sg = 1.0 / (1.0 + np.exp(-x))
    dloc = np.zeros_like(x)
    dloc[:, :, 0] = (sg[:, :, 0] - y) / (R * T)
    n1 = int(np.asarray(labels, dtype=bool).sum())
    dbce = np.zeros_like(x)
    bce = 0.0
    if NO > 1 and n1 > 0:
        bits = ((np.asarray(message, dtype=np.int64)[:, None] >> np.arange(NO - 1)) & 1).astype(np.float64)[:, None, :]
        gate = np.asarray(labels, dtype=np.float64)[:, :, None]
        bce = (bce64(x[:B, :, 1:], bits) * gate).sum() / (n1 * (NO - 1))
        dbce[:B, :, 1:] = (sg[:B, :, 1:] - bits) * gate / (n1 * (NO - 1))
    return loc, (bce if NO > 1 else None), n1, dloc, dbce


def loc_counts(logits, labels, thr, lab_rows):
    """((R, 4) {tp, fp, fn, tn}, pred bool (R, T)); labels bool (lab_rows, T) or None (all ones); NaN predicts 0"""
    x = np.asarray(logits)[:, :, 0]
    R, T = x.shape
    with np.errstate(invalid="ignore"):
        pred = x > np.float32(thr)
    y = np.ones((R, T), dtype=bool)
    if labels is not None:
        y[:] = False
        y[:lab_rows] = labels
    c = np.stack([(pred & y).sum(1), (pred & ~y).sum(1), (~pred & y).sum(1), (~pred & ~y).sum(1)], axis=1)
    return c.astype(np.int32), pred
