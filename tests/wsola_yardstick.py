"""The float64 yardstick of the pitch-preserving time stretch (wm_wsola, attacks.TimeStretch, attacks.PitchShift), written from the
definition in include/wm_hip.h with numpy alone -- nothing from the package -- and shared by tests/test_wsola_cpu.py and
tests/test_gpu_wsola.py.

  window(L)                        the rising half window, float32, entry 0 exactly 0
  frames(n_out, L), nominal(rate, K, L), positions(rate, delta, K, L, S)     K, a_k and p_k
  scores(x, q, a_k, L, S)          the float64 d(D) of every candidate D = -S .. S of one frame
  choose(d, S)                     the first of the smallest in the tie order 0, -1, +1, -2, +2, ...
  search(x, rate, n_out, L, S)     the offsets of one row from float64 scores: THE answer where every fp32 score is exact
  check_search(x, rate, delta, n_out, L, S)    a kernel's offsets frame by frame, each against the float64 scores given its predecessor
  synth / adjoint / matrix         modes 1 and 2 of one row with their per-sample bounds, and the dense (n_out, n_in) matrix
  stretch_rates, pitch_params      the draws of the two modules (the generator is tests/draw_yardstick.py's)

The bounds, with u = 2^-24 and gamma(m) = m u / (1 - m u) (Higham, Accuracy and Stability, ch. 3):
  synthesis   y = fmaf(w, u_ - v, v): the subtraction carries (1 + e1), the fmaf (1 + e2), |e| <= u, so
              |y - y64| <= u |w (u_ - v)| (1 + u) + u |y64|  <=  u (|w (u_ - v)| + |y64|) (1 + u)
  search      a term is one rounded subtraction, squared inside an fmaf; the sum has no cancellation, so whatever the order of its L - 1
              additions a computed score is d64 (1 + e), |e| <= gamma(L + 2) (two roundings of the subtraction, squared, and at most L of
              the sums; a term may also underflow, by less than 2^-126).  The kernel's choice has the smallest COMPUTED score, hence
              d64(D_k) (1 - gamma) <= dmin64 (1 + gamma) + L 2^-126.
  adjoint     F fmaf's and the one rounding of 1 - w: |dx - dx64| <= gamma(F + 2) sum |W g| over the F frames of the sample"""
import functools

import numpy as np

from draw_yardstick import WARP_PHASE, affine32, key_of, philox4x32_10, unit
from yardstick_common import U, gamma

NS = (1, 63, 255, 256, 257, 1000, 4099)
N_LONG = 16000
DIMS = ((64, 16), (256, 64), (512, 128))          # (L, S)
RATES = (0.5, 0.8, 1.0, 1.25, 2.0)
GARBAGE_RATES = (float("nan"), float("inf"), float("-inf"), 0.0, -1.0, 1e30)


# ------------------------------------------------------------------------------------------ the geometry
@functools.lru_cache(maxsize=None)
def window(L):
    hs = L // 2
    w = (0.5 - 0.5 * np.cos(np.pi * np.arange(hs) / hs)).astype(np.float32)
    w[0] = 0.0
    w.setflags(write=False)
    return w


def frames(n_out, L):
    return -(-n_out // (L // 2)) + 1


def rate_ok(rate):
    r = np.float32(rate)
    return bool(np.isfinite(r) and np.float32(0.25) <= r <= np.float32(4.0))


def nominal(rate, K, L):
    """a_k = floor(r o_k + 0.5), k < K, in float64 from the float32 rate"""
    o = (np.arange(K, dtype=np.float64) - 1.0) * (L // 2)
    return np.floor(float(np.float32(rate)) * o + 0.5).astype(np.int64)


def positions(rate, delta, K, L, S):
    """p_k = a_k + D_k with D clamped to [-S, S] and D_0 = 0"""
    d = np.clip(np.asarray(delta, dtype=np.int64), -S, S)
    d[0] = 0
    return nominal(rate, K, L) + d


def ext(x, idx):
    """x extended by zeros"""
    idx = np.asarray(idx, dtype=np.int64)
    inside = (idx >= 0) & (idx < len(x))
    out = np.zeros(idx.shape, dtype=np.float64)
    out[inside] = x[idx[inside]]
    return out


# ------------------------------------------------------------------------------------------ the search
def tie_order(S):
    """0, -1, +1, -2, +2, ..., -S, +S"""
    m = np.arange(1, S + 1)
    return np.concatenate([[0], np.stack([-m, m], axis=1).reshape(-1)])


def scores(x, q, ak, L, S):
    """d(D) = sum_j (xe[q + j] - xe[a_k + D + j])^2 for D = -S .. S, float64 from the float32 data"""
    T = ext(x, q + np.arange(L))
    C = ext(x, ak - S + np.arange(L + 2 * S))
    return ((T[None, :] - np.lib.stride_tricks.sliding_window_view(C, L)) ** 2).sum(axis=1)


def choose(d, S):
    order = tie_order(S)
    return int(order[np.argmin(d[order + S])])              # argmin: the first of the smallest


def search(x, rate, n_out, L, S):
    """the (K,) offsets of one row, chosen on float64 scores"""
    K, hs = frames(n_out, L), L // 2
    delta = np.zeros(K, dtype=np.int64)
    if not rate_ok(rate):
        return delta
    a = nominal(rate, K, L)
    p = a[0]
    for k in range(1, K):
        delta[k] = choose(scores(x, p + hs, a[k], L, S), S)
        p = a[k] + delta[k]
    return delta


def check_search(x, rate, delta, n_out, L, S):
    """Every frame k >= 1 of a kernel's offsets against the float64 scores GIVEN the kernel's own D_(k-1).  Returns (worst ratio of
    d64(D_k) to its allowance, the frames that fail).  One frame at a time on purpose: a near-tie that flips under rounding would make
    every later frame of a whole-row comparison incomparable."""
    K, hs = frames(n_out, L), L // 2
    a = nominal(rate, K, L)
    g = gamma(L + 2)
    worst, bad = 0.0, []
    assert delta[0] == 0 and (np.abs(delta) <= S).all()
    for k in range(1, K):
        d = scores(x, a[k - 1] + int(delta[k - 1]) + hs, a[k], L, S)
        dmin, got = d.min(), d[int(delta[k]) + S]
        if dmin == 0.0:
            if int(delta[k]) != choose(d, S):
                bad.append(k)
            continue
        allow = dmin * (1 + g) / (1 - g) + L * 2.0 ** -126
        worst = max(worst, (got - dmin) / (allow - dmin))
        if got > allow:
            bad.append(k)
    return worst, bad


# ------------------------------------------------------------------------------------------ synthesis, adjoint, matrix
def synth(x, rate, delta, n_out, L, S):
    """(y64, bound) of one row from given offsets (mode 1)"""
    K, hs = frames(n_out, L), L // 2
    if not rate_ok(rate):
        return np.zeros(n_out), np.zeros(n_out)
    p, w, j = positions(rate, delta, K, L, S), window(L).astype(np.float64), np.arange(hs)
    u = np.concatenate([ext(x, p[m + 1] + j) for m in range(K - 1)])
    v = np.concatenate([ext(x, p[m] + hs + j) for m in range(K - 1)])
    wd = np.tile(w, K - 1) * (u - v)
    y = wd + v
    return y[:n_out], (U * (np.abs(wd) + np.abs(y)) * (1 + U))[:n_out]


def _terms(rate, delta, n_in, n_out, L, S):
    """(s, t, W): every (input index, output index, weight) of the map inside both rows"""
    K, hs = frames(n_out, L), L // 2
    p, w = positions(rate, delta, K, L, S), window(L).astype(np.float64)
    W = np.concatenate([w, 1.0 - w])
    i = np.arange(L)
    s = (p[:, None] + i[None, :]).reshape(-1)
    t = (((np.arange(K) - 1) * hs)[:, None] + i[None, :]).reshape(-1)
    keep = (s >= 0) & (s < n_in) & (t >= 0) & (t < n_out)
    return s[keep], t[keep], np.tile(W, K)[keep]


def adjoint(g, rate, delta, n_in, L, S):
    """(dx64, bound) of one row: dx[s] = sum_k W[s - p_k] ge[o_k + s - p_k] (mode 2)"""
    if not rate_ok(rate):
        return np.zeros(n_in), np.zeros(n_in)
    s, t, W = _terms(rate, delta, n_in, len(g), L, S)
    term = W * np.asarray(g, dtype=np.float64)[t]
    F = np.bincount(s, minlength=n_in)
    return np.bincount(s, weights=term, minlength=n_in), gamma(F + 2) * np.bincount(s, weights=np.abs(term), minlength=n_in)


def matrix(rate, delta, n_in, n_out, L, S):
    """the dense (n_out, n_in) float64 matrix of mode 1, for small n"""
    M = np.zeros((n_out, n_in))
    if rate_ok(rate):
        s, t, W = _terms(rate, delta, n_in, n_out, L, S)
        np.add.at(M, (t, s), W)
    return M


# ------------------------------------------------------------------------------------------ the data
def integer_rows(n, seed):
    """two rows with integer values in [-8, 8]: one periodic (period 37, so several candidates score exactly 0 and the tie order
    decides) and one random; float32"""
    rng = np.random.default_rng(seed)
    per = np.resize(rng.integers(-8, 9, 37), n)
    return np.stack([per, rng.integers(-8, 9, n)]).astype(np.float32)


def speech_rows(rows, n, seed):
    """O(1) speech-like rows: ten harmonics of a gliding fundamental between 90 and 250 Hz at 16 kHz plus noise 26 dB below; float32"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    out = []
    for _ in range(rows):
        f0, glide = rng.uniform(90, 250), rng.uniform(-40, 40)
        phase = 2 * np.pi * (f0 * t + 0.5 * glide * t * t)
        amp = rng.uniform(0.2, 1.0, 10) / np.arange(1, 11)
        out.append(sum(a * np.sin(h * phase + rng.uniform(0, 2 * np.pi)) for h, a in zip(range(1, 11), amp)) + 0.05 * rng.standard_normal(n))
    return np.stack(out).astype(np.float32)


def hann_peak_bin(y, n_ref):
    """the peak of the Hann-windowed, eight times zero-padded DFT of y, in bins of an n_ref-point transform"""
    nfft = 8 * max(n_ref, len(y))
    spec = np.abs(np.fft.rfft(np.asarray(y, dtype=np.float64) * np.hanning(len(y)), nfft))
    return float(np.argmax(spec)) * n_ref / nfft


# ------------------------------------------------------------------------------------------ the draws (the generator is tests/draw_yardstick.py's)
def _phase_words(seed, draw, rows):
    return philox4x32_10((WARP_PHASE[0], WARP_PHASE[1], np.asarray(rows, dtype=np.uint64), int(draw)), key_of(seed))


def stretch_rates(seed, draw, rows, rate):
    """word o1 of (0xFFFFFFFC, 0xFFFFFFFF, row, draw) onto the pair `rate`; float32"""
    return affine32(rate, unit(_phase_words(seed, draw, rows)[1]))


def pitch_params(seed, draw, rows, semitones):
    """word o2 of the same counter onto the pair `semitones`; (st, beta = float32(2^(st / 12)), rate = float32(1 / beta))"""
    st = affine32(semitones, unit(_phase_words(seed, draw, rows)[2]))
    beta = (2.0 ** (st.astype(np.float64) / 12.0)).astype(np.float32)
    return st, beta, (1.0 / beta.astype(np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------ arguments the launcher refuses
_X, _R, _W, _Y, _D = 1 << 20, 1 << 24, 1 << 25, 1 << 28, 1 << 30                  # made-up, never dereferenced addresses
# wm_wsola(x, rate, win, y, delta, rows, n_in, n_out, L, S, mode, stream); at (2, 1000, 1000, 512, 128): x and y 8000 bytes, delta 2 x 5 ints
BAD_ARGS = ((_X, _R, _W, _Y, _D, 0, 1000, 1000, 512, 128, 0, None),              # rows < 1
            (_X, _R, _W, _Y, _D, 2, 0, 1000, 512, 128, 0, None),                 # n_in, n_out outside 1 .. 2^30
            (_X, _R, _W, _Y, _D, 2, 1000, 0, 512, 128, 0, None),
            (_X, _R, _W, _Y, _D, 1, (1 << 30) + 1, 1000, 512, 128, 0, None),
            (_X, _R, _W, _Y, _D, 1, 1000, (1 << 30) + 1, 512, 128, 1, None),
            (_X, _R, _W, _Y, _D, (1 << 16) + 1, 1000, 1 << 30, 512, 128, 0, None),   # rows * n above 2^46
            (_X, _R, _W, _Y, _D, 2, 1000, 1000, 32, 16, 0, None),                # L outside 64 .. 1024, or no power of two
            (_X, _R, _W, _Y, _D, 2, 1000, 1000, 2048, 128, 0, None),
            (_X, _R, _W, _Y, _D, 2, 1000, 1000, 500, 128, 0, None),
            (_X, _R, _W, _Y, _D, 2, 1000, 1000, 512, 0, 0, None),                # S outside 1 .. L / 2
            (_X, _R, _W, _Y, _D, 2, 1000, 1000, 512, 257, 0, None),
            (_X, _R, _W, _Y, _D, 2, 1000, 1000, 512, 128, -1, None),             # mode outside 0 .. 2
            (_X, _R, _W, _Y, _D, 2, 1000, 1000, 512, 128, 3, None),
            (None, _R, _W, _Y, _D, 2, 1000, 1000, 512, 128, 0, None),            # null pointers
            (_X, None, _W, _Y, _D, 2, 1000, 1000, 512, 128, 1, None),
            (_X, _R, None, _Y, _D, 2, 1000, 1000, 512, 128, 2, None),
            (_X, _R, _W, None, _D, 2, 1000, 1000, 512, 128, 0, None),
            (_X, _R, _W, _Y, None, 2, 1000, 1000, 512, 128, 0, None),
            (_X + 2, _R, _W, _Y, _D, 2, 1000, 1000, 512, 128, 0, None),          # misaligned
            (_X, _R + 1, _W, _Y, _D, 2, 1000, 1000, 512, 128, 0, None),
            (_X, _R, _W + 2, _Y, _D, 2, 1000, 1000, 512, 128, 0, None),
            (_X, _R, _W, _Y + 3, _D, 2, 1000, 1000, 512, 128, 0, None),
            (_X, _R, _W, _Y, _D + 2, 2, 1000, 1000, 512, 128, 0, None),
            (_X, _R, _W, _X, _D, 2, 1000, 1000, 512, 128, 0, None),              # in place, every mode
            (_X, _R, _W, _X, _D, 2, 1000, 1000, 512, 128, 1, None),
            (_X, _R, _W, _X, _D, 2, 1000, 1000, 512, 128, 2, None),
            (_X, _R, _W, _X + 7996, _D, 2, 1000, 1000, 512, 128, 0, None),       # y overlaps the last float of x
            (_X, _R, _W, _X + 7996, _D, 2, 2000, 1000, 512, 128, 2, None),       # mode 2: x is the (2, 1000) gradient
            (_X, _Y + 4, _W, _Y, _D, 2, 1000, 1000, 512, 128, 0, None),          # the rates inside y
            (_X, _R, _Y - 1020, _Y, _D, 2, 1000, 1000, 512, 128, 0, None),       # y overlaps the window's last entry
            (_X, _R, _W, _Y, _Y + 7996, 2, 1000, 1000, 512, 128, 1, None),       # delta overlaps y
            (_X, _R, _W, _Y, _Y - 36, 2, 1000, 1000, 512, 128, 2, None),
            (_X, _R, _W, _Y, _X + 400, 2, 1000, 1000, 512, 128, 0, None),        # mode 0 writes delta: inside x, on the rates, on the window
            (_X, _R, _W, _Y, _R + 4, 2, 1000, 1000, 512, 128, 0, None),
            (_X, _R, _W, _Y, _W - 36, 2, 1000, 1000, 512, 128, 0, None))
