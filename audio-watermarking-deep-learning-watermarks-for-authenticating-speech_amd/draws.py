"""The attacks' counter-based draws, restated on the host: the numbers the kernels draw, from numpy alone.

The noise is counter-based (Philox4x32-10 -> Box-Muller), so nothing is stored for the backward pass, a run is reproducible from `seed`,
and philox4x32_10 / normal_noise below restate on the host exactly the numbers the kernel draws.  Two tables keep the attacks apart:

  FAMILIES   name -> (word 0, word 1) of the Philox counter (word 0, word 1, row, draw).  No two families share a counter.
  WORDS      (family, output word) -> the one parameter that word is drawn for, "Owner.parameter".  A cell that is not there is free.

Every row_* function below asks WORDS for its word by the parameter's name (_owned); none of them holds a word index.  A new attack
takes a free cell of WORDS, or a new family, and adds its row to tests/test_draws_layout_cpu.py."""
from __future__ import annotations

import math

import numpy as np

from . import dsp

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
# The counter families: name -> (word 0, word 1) of the Philox counter (word 0, word 1, row, draw).  None is a word that counts: t >> 2 of
# a row's samples (n <= 2^34, so below 2^32) and k >> 2 of a response's taps (below 2^12).  No two families share a counter, and
# csrc/distort.hip and csrc/splice.hip spell the same words.
FAMILIES = {
    "sample": (None, 0),
    "rir_tap": (None, 0xFFFFFFFE),
    "param": (0xFFFFFFFF, 0xFFFFFFFF),
    "param2": (0xFFFFFFFE, 0xFFFFFFFF),
    "warp": (0xFFFFFFFD, 0xFFFFFFFF),
    "warp_phase": (0xFFFFFFFC, 0xFFFFFFFF),
    **{f"splice_span{j}": (0xFFFFFFFB - 2 * j, 0xFFFFFFFF) for j in range(dsp.SPLICE_MAX_SPANS)},
    **{f"splice_shift{j}": (0xFFFFFFFA - 2 * j, 0xFFFFFFFF) for j in range(dsp.SPLICE_MAX_SPANS)},
}
# Every output word in use: (family, word 0..3) -> its one owner.  "sample" and "rir_tap" yield normals from all four words and are not here.
WORDS = {
    ("param", 0): "Distortion.gain_db", ("param", 1): "Distortion.snr_db", ("param", 2): "Distortion.noisy",
    ("param", 3): "TransformCodec.snr_db",
    ("param2", 0): "Reverb.rt60", ("param2", 1): "Reverb.drr_db", ("param2", 2): "Convolved.bank", ("param2", 3): "LpcCodec.snr_db",
    ("warp", 0): "TimeWarp.speed", ("warp", 1): "TimeWarp.shift_s", ("warp", 2): "TimeWarp.flutter_hz",
    ("warp", 3): "TimeWarp.flutter_depth",
    ("warp_phase", 0): "TimeWarp.phase", ("warp_phase", 1): "TimeStretch.rate", ("warp_phase", 2): "PitchShift.semitones",
    ("warp_phase", 3): "NoiseSuppress.reduce_db",
    **{(f"splice_span{j}", k): f"Splice.{p}[{j}]" for j in range(dsp.SPLICE_MAX_SPANS)
       for k, p in enumerate(("coin", "length", "start", "kind"))},
    **{(f"splice_shift{j}", 0): f"Splice.shift[{j}]" for j in range(dsp.SPLICE_MAX_SPANS)},
}
_CELL = {owner: cell for cell, owner in WORDS.items()}


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11).  counter: four uint32 values or arrays that
    broadcast together, key: two uint32 values.  Returns a uint32 array of shape (4, ...): the four output words."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for v in counter]
    if len(c) != 4 or len(key) != 2:
        raise ValueError("philox4x32_10: a counter of four words and a key of two")
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(k) & 0xFFFFFFFF for k in key)
    lo = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]                     # 32 x 32 bits: exact in 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c).astype(np.uint32)


def _unit(o):
    """u = ((o >> 9) + 0.5) * 2^-23: 24 bits, exact in float32 (and float64), never 0 or 1"""
    return ((o >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def _key(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed & 0xFFFFFFFF, seed >> 32


def _words(family, seed, draw, rows, count=None):
    """The four Philox output words of `family` for the rows `rows` (an int or an int array of row0 + r) of (seed, draw); count: the values
    of the word that counts, for the families that have one"""
    w0, w1 = FAMILIES[family]
    return philox4x32_10((count if w0 is None else w0, w1, np.asarray(rows, dtype=np.uint64), int(draw)), _key(seed))


def _owned(seed, draw, rows, *owners):
    """The output words WORDS gives the parameters `owners`, in their order, for the rows `rows` of (seed, draw).  The owners share one
    family, which is evaluated once."""
    (family,) = {_CELL[owner][0] for owner in owners}
    o = _words(family, seed, draw, rows)
    return [o[_CELL[owner][1]] for owner in owners]


def _affine(pair, u):
    """fmaf(high - low, u, low) as the kernels form it: float32 bounds, the product exact in float64, one rounding to float32"""
    lo, hi = (np.float32(v) for v in pair)
    return (np.float64(hi - lo) * u + np.float64(lo)).astype(np.float32)


def normal_noise(seed, draw, row, n):
    """z(seed, draw, row, t) for t < n as a float64 array: counter (q, 0, row, draw) with q = t >> 2, key (seed low, seed high);
    words (o0, o1) give sqrt(-2 ln u(o0)) * (cos, sin)(2 pi u(o1)) for samples 4q and 4q+1, (o2, o3) the same for 4q+2 and 4q+3."""
    return _normals(seed, draw, row, n, "sample")


def _normals(seed, draw, row, n, family):
    """normal_noise from the counting family `family`: "sample" or "rir_tap" """
    n = int(n)
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    o = _words(family, seed, draw, int(row), q)
    z = np.empty((len(q), 4), dtype=np.float64)
    for p in (0, 1):
        rad, th = np.sqrt(-2.0 * np.log(_unit(o[2 * p]))), 2.0 * math.pi * _unit(o[2 * p + 1])
        z[:, 2 * p], z[:, 2 * p + 1] = rad * np.cos(th), rad * np.sin(th)
    return z.reshape(-1)[:n]


def row_parameters(seed, draw, rows, bounds):
    """(gain_db, snr_db, noisy) of rows `rows` (an int array of row0 + r), as the kernel draws them: float32 arrays and a bool array"""
    bounds, (gain, snr, coin) = tuple(bounds), _owned(seed, draw, rows, "Distortion.gain_db", "Distortion.snr_db", "Distortion.noisy")
    return _affine(bounds[0:2], _unit(gain)), _affine(bounds[2:4], _unit(snr)), _unit(coin) < np.float64(np.float32(bounds[4]))


def row_snr_db(seed, draw, rows, snr_db):
    """TransformCodec's per-row quality for rows `rows` (an int array of row0 + r), a float32 array: its word of the counter Distortion
    draws a row's parameters from, mapped onto the pair snr_db as fmaf(high - low, u, low)"""
    return _affine(snr_db, _unit(*_owned(seed, draw, rows, "TransformCodec.snr_db")))


def row_lpc_snr_db(seed, draw, rows, snr_db):
    """LpcCodec's per-row quality for rows `rows` (an int array of row0 + r), a float32 array: its word of the "param2" counter, mapped
    onto the pair snr_db as fmaf(high - low, u, low)"""
    return _affine(snr_db, _unit(*_owned(seed, draw, rows, "LpcCodec.snr_db")))


def row_reduce_db(seed, draw, rows, reduce_db):
    """NoiseSuppress's per-row depth for rows `rows` (an int array of row0 + r), a float32 array: its word of the "warp_phase" counter,
    mapped onto the pair reduce_db as fmaf(high - low, u, low)"""
    return _affine(reduce_db, _unit(*_owned(seed, draw, np.asarray(rows, dtype=np.uint64), "NoiseSuppress.reduce_db")))


def row_reverb_params(seed, draw, rows, rt60, drr_db):
    """Reverb's (rt60, drr_db) of rows `rows` (an int array of row0 + r), two float32 arrays: its two words of the counter
    (0xFFFFFFFE, 0xFFFFFFFF, row, draw), mapped onto the pairs as fmaf(high - low, u, low) in float32"""
    o_rt60, o_drr = _owned(seed, draw, rows, "Reverb.rt60", "Reverb.drr_db")
    return _affine(rt60, _unit(o_rt60)), _affine(drr_db, _unit(o_drr))


def row_bank_index(seed, draw, rows, entries):
    """Convolved's choice among `entries` responses for rows `rows`: floor(u * entries) with its word of the same counter, an int64 array"""
    return np.floor(_unit(*_owned(seed, draw, rows, "Convolved.bank")) * int(entries)).astype(np.int64)


def rir_taps(seed, draw, row, rt60, drr_db, K, sample_rate):
    """The synthetic response wm_rir_synth gives row `row` (= row0 + r), restated in float64: e[0] = 0, e[k] = z_k exp(-k c) with
    c = 3 ln 10 / (rt60 * sample_rate) and z_k the normal of "sample" k of the counter (k >> 2, 0xFFFFFFFE, row, draw);
    h[0] = 1 / sqrt(1 + w), h[k] = sqrt(w / sum e^2) e[k] / sqrt(1 + w), w = 10^(-drr_db / 10).  rt60 and drr_db enter as float32 values,
    drr_db clamped to [-100, 100]; K = 1, sum e^2 = 0, rt60 not > 0 or a non-finite drr_db give {1, 0, ...}."""
    K = int(K)
    rt60, drr_db = float(np.float32(rt60)), float(np.float32(drr_db))
    h = np.zeros(K, dtype=np.float64)
    h[0] = 1.0
    if K == 1 or not rt60 > 0.0 or not math.isfinite(drr_db):
        return h
    c = 3.0 * math.log(10.0) / (rt60 * float(np.float32(sample_rate)))
    e = _normals(seed, draw, row, K, "rir_tap") * np.exp(-np.arange(K, dtype=np.float64) * c)
    e[0] = 0.0
    E = float(np.sum(e * e))
    if not E > 0.0:
        return h
    w = 10.0 ** (-min(max(drr_db, -100.0), 100.0) / 10.0)
    h = math.sqrt(w / E) * e / math.sqrt(1.0 + w)
    h[0] = 1.0 / math.sqrt(1.0 + w)
    return h


def row_warp_params(seed, draw, rows, speed, shift_s, flutter_hz, flutter_depth, sample_rate):
    """TimeWarp's (len(rows), 6) float32 parameters {a, off, d, w, phi, c} of rows `rows` (an int array of row0 + r), the rows of
    wm_time_warp's `params`.  speed, shift_s, flutter_hz, flutter_depth: (low, high) pairs (the last two None: no flutter).  The four words
    of the counter (0xFFFFFFFD, 0xFFFFFFFF, row, draw) map onto speed, shift, flutter rate and flutter depth as
    fmaf(high - low, u, low) in float32, TimeWarp's word of (0xFFFFFFFC, 0xFFFFFFFF, row, draw) is the phase u.  From these float32 draws, in
    float64 and rounded to float32 once each: a = speed, off = shift * sample_rate, w = rate / sample_rate, d = depth a / (2 pi w) with the
    rounded w (0 where w or depth is 0), phi = u, c = min(1, 1 / (a (1 + depth)))."""
    rows = np.asarray(rows, dtype=np.uint64)
    o_speed, o_shift, o_hz, o_depth = _owned(seed, draw, rows, "TimeWarp.speed", "TimeWarp.shift_s", "TimeWarp.flutter_hz",
                                             "TimeWarp.flutter_depth")
    phase = _unit(*_owned(seed, draw, rows, "TimeWarp.phase"))
    flutter = flutter_hz is not None and flutter_depth is not None
    a = _affine(speed, _unit(o_speed)).astype(np.float64)
    shift = _affine(shift_s, _unit(o_shift)).astype(np.float64)
    hz = _affine(flutter_hz, _unit(o_hz)).astype(np.float64) if flutter else np.zeros(len(rows))
    depth = _affine(flutter_depth, _unit(o_depth)).astype(np.float64) if flutter else np.zeros(len(rows))
    w = (hz / float(sample_rate)).astype(np.float32)
    on = (w != 0) & (depth != 0)
    d = np.where(on, depth * a / (2.0 * math.pi * np.where(on, w.astype(np.float64), 1.0)), 0.0)
    c = np.minimum(1.0, 1.0 / (a * (1.0 + depth)))
    return np.stack([a, shift * float(sample_rate), d, w.astype(np.float64), np.where(on, phase, 0.0), c], axis=1).astype(np.float32)


def row_stretch_rates(seed, draw, rows, rate):
    """TimeStretch's float32 rate of rows `rows` (an int array of row0 + r): its word of the counter (0xFFFFFFFC, 0xFFFFFFFF, row, draw)
    onto the pair `rate` as fmaf(high - low, u, low) in float32"""
    return _affine(rate, _unit(*_owned(seed, draw, np.asarray(rows, dtype=np.uint64), "TimeStretch.rate")))


def row_pitch_params(seed, draw, rows, semitones):
    """PitchShift's (semitones, beta, rate) of rows `rows`, three float32 arrays: its word of the counter (0xFFFFFFFC, 0xFFFFFFFF, row,
    draw) onto the pair `semitones` as fmaf(high - low, u, low) in float32; beta = float32(2^(st / 12)) and rate = float32(1 / beta), each
    formed in float64 from the float32 value before it"""
    st = _affine(semitones, _unit(*_owned(seed, draw, np.asarray(rows, dtype=np.uint64), "PitchShift.semitones")))
    beta = np.exp2(st.astype(np.float64) / 12.0).astype(np.float32)
    return st, beta, (1.0 / beta.astype(np.float64)).astype(np.float32)


SPLICE_KINDS = ("original", "silence", "moved")           # the `kind` of a span: 0, 1, 2


def _check_cut(n, max_spans, p_span, len_lo, len_hi, p_original, p_silence):
    n = int(n)
    if not 1 <= n <= dsp.SPLICE_MAX_N:
        raise ValueError(f"n: expected 1 <= n <= 2^24 samples, got {n}")
    if isinstance(max_spans, bool) or not isinstance(max_spans, (int, np.integer)) or not 1 <= max_spans <= dsp.SPLICE_MAX_SPANS:
        raise ValueError(f"max_spans: expected an int in [1, {dsp.SPLICE_MAX_SPANS}], got {max_spans!r}")
    if not 1 <= int(len_lo) <= int(len_hi) <= n:
        raise ValueError(f"span lengths: expected 1 <= len_lo <= len_hi <= n = {n} samples, got {len_lo!r} and {len_hi!r}")
    p = [np.float32(v) for v in (p_span, p_original, p_silence)]
    if not all(0.0 <= float(v) <= 1.0 for v in p) or float(p[1]) + float(p[2]) > 1.0:
        raise ValueError(f"probabilities: expected p_span, p_original, p_silence in [0, 1] with p_original + p_silence <= 1 (as float32 "
                         f"values), got {p_span!r}, {p_original!r}, {p_silence!r}")
    return n, int(max_spans), int(len_lo), int(len_hi), float(p[0]), float(p[1]), float(p[1]) + float(p[2])


def row_splice_spans(seed, draw, rows, n, max_spans=2, p_span=0.5, len_lo=800, len_hi=6400, p_original=1 / 3, p_silence=1 / 3):
    """The spans wm_splice draws for rows `rows` (an int array of row0 + r) of n samples: per row a list of max_spans tuples
    (start, L, kind, shift, active), ints and a bool, kind an index into SPLICE_KINDS.  Span j takes the four words (coin, length, start,
    kind) of the counter (0xFFFFFFFB - 2j, 0xFFFFFFFF, row, draw) and the word (shift) of (0xFFFFFFFA - 2j, 0xFFFFFFFF, row, draw): active
    iff u(coin) < p_span, L = len_lo + ((v(length) (len_hi - len_lo + 1)) >> 23), start = (v(start) (n - L + 1)) >> 23, kind from u(kind)
    against p_original and p_original + p_silence, shift = 1 + ((v(shift) (n - 1)) >> 23), with v(o) = o >> 9 and u = (v + 0.5) 2^-23.
    The probabilities enter as float32 values and are compared in float64, the products are integers: nothing is rounded.  n = 1: "moved"
    is reported, and acts, as "original".  An inactive span keeps the geometry it drew."""
    n, max_spans, len_lo, len_hi, p_span, t_original, t_silence = _check_cut(n, max_spans, p_span, len_lo, len_hi, p_original, p_silence)
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1)
    out = [[] for _ in rows]
    for j in range(max_spans):
        o = _owned(seed, draw, rows, *(f"Splice.{p}[{j}]" for p in ("coin", "length", "start", "kind")))
        (o2,) = _owned(seed, draw, rows, f"Splice.shift[{j}]")
        for i in range(len(rows)):
            v_coin, v_length, v_start, v_kind = (int(w[i]) >> 9 for w in o)
            L = len_lo + ((v_length * (len_hi - len_lo + 1)) >> 23)
            start = (v_start * (n - L + 1)) >> 23
            u3 = (v_kind + 0.5) * 2.0 ** -23
            kind = 0 if u3 < t_original else (1 if u3 < t_silence else 2)
            if n == 1 and kind == 2:
                kind = 0
            shift = 1 + (((int(o2[i]) >> 9) * (n - 1)) >> 23)
            out[i].append((start, L, kind, shift, bool((v_coin + 0.5) * 2.0 ** -23 < p_span)))
    return out
