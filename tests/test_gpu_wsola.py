"""wm_wsola / ops.wsola / ops.WsolaFn / attacks.TimeStretch / attacks.PitchShift on the GPU against the float64 yardstick of
tests/wsola_yardstick.py (numpy from the definition in include/wm_hip.h; nothing from the package).  Kernel-level cases: n in {1, 63, 255,
256, 257, 1000, 4099, 16000}, (L, S) in {(64, 16), (256, 64), (512, 128)}, rates {0.5, 0.8, 1, 1.25, 2}, three rows a launch, every buffer
4 bytes off an 8-byte boundary, one guard word either side of y and of delta in every launch (`raw` below).

Tolerances (none tuned to the kernel; the yardstick's docstring derives them):
  identity    rate 1: bit for bit, delta all zero.
  synthesis   |y - y64| <= u (|w (u_ - v)| + |y64|) (1 + u), u = 2^-24: one subtraction and one fmaf.
  search      integer data in [-8, 8] (every fp32 score exact in any order, L * 256 < 2^24): delta equals the yardstick's, frame for frame.
              floats: for every frame, given the kernel's own predecessor, d64(D_k) <= min d64 (1 + g) / (1 - g) + L 2^-126, g = gamma(L + 2);
              where min d64 is 0 the first zero-score candidate of the tie order.
  adjoint     |dx - dx64| <= gamma(F + 2) sum |W g| over the F frames of a sample; |<Wu, v> - <u, W^T v>| within the two bounds carried
              through the inner products.
Every reference is computed once per case and never written to.

Measured on an MI355X (largest err / bound per test, printed by every case): see DESIGN.md section 4n."""
import os

import numpy as np
import pytest
import torch

from oracle import wm_oracle as O

import wsola_yardstick as Y
from gpu_support import awm, dev  # noqa: F401
from gpu_support import bits, reference_models, st, to_dev

pytestmark = pytest.mark.gpu

ALL_N = Y.NS + (Y.N_LONG,)
SIX_RATES = Y.RATES + (1.1,)                          # two launches of three rows


def off4(a, dev, dtype=torch.float32):
    """the same values in a buffer that starts 4 bytes earlier: the returned tensor's pointer is 4 (mod 8)"""
    a = torch.from_numpy(np.array(a)).to(dtype).reshape(-1)          # a copy: the yardstick's arrays are read-only
    buf = torch.empty(a.numel() + 1, dtype=dtype, device=dev)
    buf[1:] = a.to(dev)
    assert buf[1:].data_ptr() % 8 == 4
    return buf[1:]


def raw(awm, dev, mode, x, rates, n_res, L, S, delta=None, win=None):
    """One wm_wsola launch on numpy rows: x (rows, n), n_res samples a row of the result (mode 2: x is the gradient, n_res the forward
    call's n_in).  x, rate, win, y and delta all start 4 bytes off an 8-byte boundary; one guard float either side of y and one guard
    int either side of delta are checked.  Returns (y, delta) as numpy."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, n = x.shape
    n_in, n_out = (n_res, n) if mode == 2 else (n, n_res)
    K = Y.frames(n_out, L)
    xb, rb, wb = off4(x, dev), off4(np.asarray(rates, dtype=np.float32), dev), off4(Y.window(L) if win is None else win, dev)
    ybuf = torch.full((rows * n_res + 2,), 12345.0, device=dev)
    dbuf = torch.full((rows * K + 2,), 777, dtype=torch.int32, device=dev)
    if delta is not None:
        dbuf[1:-1] = torch.as_tensor(np.ascontiguousarray(delta)).to(torch.int32).reshape(-1).to(dev)
    assert (ybuf.data_ptr() + 4) % 8 == 4 and (dbuf.data_ptr() + 4) % 8 == 4
    awm.lib.wm_wsola(xb.data_ptr(), rb.data_ptr(), wb.data_ptr(), ybuf.data_ptr() + 4, dbuf.data_ptr() + 4, rows, n_in, n_out, L, S, mode, st())
    torch.cuda.synchronize()
    assert float(ybuf[0]) == 12345.0 and float(ybuf[-1]) == 12345.0 and int(dbuf[0]) == 777 and int(dbuf[-1]) == 777, "guards"
    d = dbuf[1:-1].view(rows, K).cpu().numpy()
    if delta is not None:
        assert np.array_equal(d, np.asarray(delta).reshape(rows, K)), "modes 1 and 2 only read delta"
    return ybuf[1:-1].view(rows, n_res).cpu().numpy(), d


def by_threes(awm, dev, mode, x, rates, n_res, L, S, delta=None):
    """launches of three rows (the last one padded with the first rows)"""
    ys, ds = [], []
    for r0 in range(0, len(x), 3):
        idx = [(r0 + i) % len(x) for i in range(3)]
        y, d = raw(awm, dev, mode, x[idx], np.asarray(rates)[idx], n_res, L, S, None if delta is None else np.asarray(delta)[idx])
        keep = min(3, len(x) - r0)
        ys.append(y[:keep]); ds.append(d[:keep])
    return np.concatenate(ys), np.concatenate(ds)


def ratio(err, bnd):
    return float((err / np.maximum(bnd, 1e-300)).max()) if (bnd > 0).any() else 0.0


# ------------------------------------------------------------------------------------------ 1. identity, bit for bit
@pytest.mark.parametrize("L,S", Y.DIMS)
@pytest.mark.parametrize("n", ALL_N)
def test_rate_one_is_the_identity_bit_for_bit(awm, dev, n, L, S):
    x = np.random.default_rng(n + L).standard_normal((3, n)).astype(np.float32)
    x[1, n // 3:n // 2] = 0.0                                # a silent stretch: every candidate there scores 0, the tie order keeps D = 0
    x[1, (2 * n) // 3:] = 0.0
    x[2] = 0.0
    for n_out in (n, n + 70, max(1, n - 40)):
        y, delta = raw(awm, dev, 0, x, [1.0, 1.0, 1.0], n_out, L, S)
        want = np.zeros((3, n_out), dtype=np.float32)
        want[:, :min(n, n_out)] = x[:, :min(n, n_out)]
        assert np.array_equal(y.view(np.int32), want.view(np.int32)), f"n {n} n_out {n_out}: y is x, truncated or zero-padded"
        assert not delta.any()


# ------------------------------------------------------------------------------------------ 2. synthesis from given offsets
@pytest.mark.parametrize("L,S", Y.DIMS)
@pytest.mark.parametrize("n", ALL_N)
def test_synthesis_against_float64(awm, dev, n, L, S):
    rng = np.random.default_rng(11 * n + S)
    x = rng.standard_normal((6, n)).astype(np.float32)
    worst = 0.0
    for n_out in (n, n + 100):
        delta = rng.integers(-S - 5, S + 6, (6, Y.frames(n_out, L))).astype(np.int32)      # a few beyond [-S, S]: clamped on load
        y, _ = by_threes(awm, dev, 1, x, SIX_RATES, n_out, L, S, delta)
        for r, rate in enumerate(SIX_RATES):
            ref, bnd = Y.synth(x[r], rate, delta[r], n_out, L, S)
            err = np.abs(y[r] - ref)
            worst = max(worst, ratio(err, bnd))
            assert (err <= bnd).all(), f"n {n} n_out {n_out} ({L}, {S}) rate {rate}: err / bound {ratio(err, bnd):.3f} at {np.argmax(err - bnd)}"
        assert n < 257 or np.abs(y).max() > 0.5
    print(f"n {n} ({L}, {S}): synthesis worst err / bound {worst:.4f}")


# ------------------------------------------------------------------------------------------ 3. the search where every score is exact
@pytest.mark.parametrize("L,S", Y.DIMS)
@pytest.mark.parametrize("n", ALL_N)
def test_search_on_integers_is_the_yardsticks(awm, dev, n, L, S):
    two = Y.integer_rows(n, 100 * n + L)
    x = np.concatenate([two] * len(Y.RATES))                 # (periodic, random) at every rate
    rates = np.repeat(Y.RATES, 2)
    for n_out in (n, (3 * n) // 2 + 5):
        y, delta = by_threes(awm, dev, 0, x, rates, n_out, L, S)
        for r, rate in enumerate(rates):
            want = Y.search(x[r], rate, n_out, L, S)
            assert np.array_equal(delta[r], want), (f"n {n} n_out {n_out} ({L}, {S}) rate {rate} {'periodic' if r % 2 == 0 else 'random'}: "
                                                    f"first at frame {np.argmax(delta[r] != want)}: {delta[r][:8]} vs {want[:8]}")
            ref, bnd = Y.synth(x[r], rate, want, n_out, L, S)
            assert (np.abs(y[r] - ref) <= bnd).all()
    if n >= 1000:
        assert len(np.unique(delta)) > 3, "the search moves"


# ------------------------------------------------------------------------------------------ 4. the search on floats, frame by frame
@pytest.mark.parametrize("L,S", Y.DIMS)
@pytest.mark.parametrize("n", ALL_N)
def test_search_on_floats_frame_by_frame(awm, dev, n, L, S):
    x = Y.speech_rows(6, n, 7 * n + L)
    y, delta = by_threes(awm, dev, 0, x, SIX_RATES, n, L, S)
    worst, frames = 0.0, 0
    for r, rate in enumerate(SIX_RATES):
        w, bad = Y.check_search(x[r], rate, delta[r], n, L, S)
        worst, frames = max(worst, w), frames + len(delta[r]) - 1
        assert not bad, f"n {n} ({L}, {S}) rate {rate}: frames {bad[:5]} chose a candidate beyond the rounding of the best one"
        ref, bnd = Y.synth(x[r], rate, delta[r], n, L, S)
        assert (np.abs(y[r] - ref) <= bnd).all()
    print(f"n {n} ({L}, {S}): {frames} frames, worst (d64(D_k) - dmin) / allowance {worst:.4f}")


# ------------------------------------------------------------------------------------------ 5. the adjoint
@pytest.mark.parametrize("L,S", Y.DIMS)
@pytest.mark.parametrize("n", ALL_N)
def test_adjoint_against_float64_and_the_identity(awm, dev, n, L, S):
    rng = np.random.default_rng(13 * n + L)
    u = Y.speech_rows(6, n, 3 * n + S)
    worst = worst_id = 0.0
    for n_out in (n, n + 100):
        v = rng.standard_normal((6, n_out)).astype(np.float32)
        Wu, delta = by_threes(awm, dev, 0, u, SIX_RATES, n_out, L, S)
        Wtv, _ = by_threes(awm, dev, 2, v, SIX_RATES, n, L, S, delta)
        for r, rate in enumerate(SIX_RATES):
            ref, bnd = Y.adjoint(v[r], rate, delta[r], n, L, S)
            err = np.abs(Wtv[r] - ref)
            worst = max(worst, ratio(err, bnd))
            assert (err <= bnd).all(), f"n {n} n_out {n_out} ({L}, {S}) rate {rate}: err / bound {ratio(err, bnd):.3f} at {np.argmax(err - bnd)}"
            _, fb = Y.synth(u[r], rate, delta[r], n_out, L, S)
            lhs, rhs = float((Wu[r].astype(np.float64) * v[r]).sum()), float((u[r].astype(np.float64) * Wtv[r]).sum())
            room = float((np.abs(v[r]) * fb).sum() + (np.abs(u[r]) * bnd).sum())
            if room > 0:
                worst_id = max(worst_id, abs(lhs - rhs) / room)
            assert abs(lhs - rhs) <= room, f"n {n} ({L}, {S}) rate {rate}: |<Wu, v> - <u, W^T v>| = {abs(lhs - rhs):.3e} > {room:.3e}"
    print(f"n {n} ({L}, {S}): adjoint worst err / bound {worst:.4f}, identity {worst_id:.4f}")


# ------------------------------------------------------------------------------------------ 6. independent rows, reproducible launches
@pytest.mark.parametrize("L,S", Y.DIMS)
@pytest.mark.parametrize("n", [63, 257, 4099])
def test_rows_are_independent_and_launches_reproducible(awm, dev, n, L, S):
    x = Y.speech_rows(3, n, 5 * n + L)
    rates = [0.8, 1.25, 1.1]
    g = np.random.default_rng(n).standard_normal((3, n)).astype(np.float32)
    y, delta = raw(awm, dev, 0, x, rates, n, L, S)
    dx, _ = raw(awm, dev, 2, g, rates, n, L, S, delta)
    y2, delta2 = raw(awm, dev, 0, x, rates, n, L, S)
    assert np.array_equal(y.view(np.int32), y2.view(np.int32)) and np.array_equal(delta, delta2), "two launches give identical bits"
    assert np.array_equal(dx.view(np.int32), raw(awm, dev, 2, g, rates, n, L, S, delta)[0].view(np.int32))
    assert np.array_equal(raw(awm, dev, 1, x, rates, n, L, S, delta)[0].view(np.int32), y.view(np.int32)), "mode 1 on mode 0's offsets is mode 0"
    for r in range(3):
        y1, d1 = raw(awm, dev, 0, x[r:r + 1], rates[r:r + 1], n, L, S)
        assert np.array_equal(y1[0].view(np.int32), y[r].view(np.int32)) and np.array_equal(d1[0], delta[r]), f"row {r} alone equals row {r} of the batch"
        dx1, _ = raw(awm, dev, 2, g[r:r + 1], rates[r:r + 1], n, L, S, delta[r:r + 1])
        assert np.array_equal(dx1[0].view(np.int32), dx[r].view(np.int32))
    xn = x.copy()
    xn[1] = np.nan
    yn, dn = raw(awm, dev, 0, xn, rates, n, L, S)
    assert np.array_equal(yn[[0, 2]].view(np.int32), y[[0, 2]].view(np.int32)) and np.array_equal(dn[[0, 2]], delta[[0, 2]]), "a row of NaN"
    assert (np.abs(dn[1]) <= S).all()
    garbage = np.where(np.arange(delta.size).reshape(delta.shape) % 2 == 0, 2 ** 31 - 1, -2 ** 31).astype(np.int32)
    garbage[[0, 2]] = delta[[0, 2]]
    for bad in Y.GARBAGE_RATES + (0.2, 4.5):
        rg = [rates[0], bad, rates[2]]
        yg, dg = raw(awm, dev, 0, x, rg, n, L, S)
        assert np.array_equal(yg[[0, 2]].view(np.int32), y[[0, 2]].view(np.int32)) and np.array_equal(dg[[0, 2]], delta[[0, 2]]), f"rate {bad}"
        assert not yg[1].any() and not dg[1].any(), f"rate {bad}: the row is zeros, in y and in delta"
        for mode, src in ((1, x), (2, g)):
            og, _ = raw(awm, dev, mode, src, rg, n, L, S, garbage)
            want = y if mode == 1 else dx
            assert np.array_equal(og[[0, 2]].view(np.int32), want[[0, 2]].view(np.int32)) and not og[1].any(), f"mode {mode}, rate {bad}"
    # garbage offsets at a good rate: clamped, bounded, the neighbours untouched
    for mode, src in ((1, x), (2, g)):
        og, _ = raw(awm, dev, mode, src, rates, n, L, S, garbage)
        want = y if mode == 1 else dx
        assert np.array_equal(og[[0, 2]].view(np.int32), want[[0, 2]].view(np.int32)) and np.isfinite(og[1]).all()
        ref, bnd = (Y.synth(x[1], rates[1], garbage[1], n, L, S) if mode == 1 else Y.adjoint(g[1], rates[1], garbage[1], n, L, S))
        assert (np.abs(og[1] - ref) <= bnd).all(), "offsets beyond [-S, S] are clamped on load"


# ------------------------------------------------------------------------------------------ 7. it is what it claims to be
N_TONE, BIN = 4096, 100.37


def tone():
    return np.sin(2 * np.pi * BIN * np.arange(N_TONE) / N_TONE + 0.3).astype(np.float32)


@pytest.mark.parametrize("L,S", [(256, 64), (512, 128)])
def test_a_stretch_keeps_the_pitch_and_a_warp_moves_it(awm, dev, L, S):
    x = np.stack([tone()] * 3)
    rates = [0.8, 1.25, 1.0]
    y, delta = raw(awm, dev, 0, x, rates, N_TONE, L, S)
    for r, rate in enumerate(rates):
        cov = min(N_TONE, int((N_TONE - L - S) / rate))           # the part of the output whose frames lie inside the input
        peak = Y.hann_peak_bin(y[r][:cov], N_TONE)
        warped = awm.TimeWarp(speed=rate)(to_dev(x[r], dev)).cpu().numpy()
        wpeak = Y.hann_peak_bin(warped[:min(N_TONE, int((N_TONE - 20) / rate))], N_TONE)
        print(f"({L}, {S}) rate {rate}: stretch peak at bin {peak:.2f} (the tone: {BIN}), TimeWarp's at {wpeak:.2f} (rate * tone: {rate * BIN:.2f})")
        assert abs(peak - BIN) <= 1.0, "the stretch keeps the spectrum"
        assert abs(wpeak - rate * BIN) <= 1.0, "the speed change moves it with the rate"
        assert rate == 1.0 or delta[r].any()


@pytest.mark.parametrize("semitones", [-3.0, 2.0])
def test_pitch_shift_moves_the_peak_by_the_interval(awm, dev, semitones):
    L = 512
    y = awm.PitchShift(semitones=semitones)(to_dev(tone(), dev)).cpu().numpy()
    peak, want = Y.hann_peak_bin(y[L:N_TONE - L], N_TONE), 2.0 ** (semitones / 12.0) * BIN
    print(f"{semitones} semitones: peak at bin {peak:.2f}, 2^(s / 12) * tone = {want:.2f}")
    assert y.shape == (N_TONE,) and abs(peak - want) <= 1.0


@pytest.mark.parametrize("L,S", Y.DIMS)
def test_support_stays_within_the_search_range_of_its_place(awm, dev, L, S):
    """|p_k - r o_k| <= S + 1/2, so y[t] reads x within |1 - r| L + S + 1/2 of r t"""
    n, t0, W = 4096, 1500, 300
    x = np.zeros((6, n), dtype=np.float32)
    x[:, t0:t0 + W] = np.random.default_rng(L).uniform(0.5, 1.0, (6, W)) * np.random.default_rng(S).choice([-1.0, 1.0], (6, W))
    y, _ = by_threes(awm, dev, 0, x, SIX_RATES, n, L, S)
    for r, rate in enumerate(SIX_RATES):
        B = abs(1 - rate) * L + S + 1
        nz = np.flatnonzero(y[r])
        assert len(nz) > W / rate / 2 and (t0 - B) / rate <= nz[0] and nz[-1] <= (t0 + W + B) / rate, f"({L}, {S}) rate {rate}: [{nz[0]}, {nz[-1]}]"
    if (L, S) == (512, 128):
        for semitones in (-3.0, 2.0):
            att = awm.PitchShift(semitones=semitones)
            z = att(to_dev(x[0], dev)).cpu().numpy()
            beta, rate = float(att.last_params[0, 1]), float(att.last_params[0, 2])
            B = abs(1 - rate) * L + S + 1 + 16 * max(1.0, 1.0 / beta) + 1       # and the interpolator's half width, in output samples
            nz = np.flatnonzero(z)
            assert len(nz) > W / 2 and t0 - B <= nz[0] and nz[-1] <= t0 + W + B, f"{semitones} semitones: [{nz[0]}, {nz[-1]}]"


# ------------------------------------------------------------------------------------------ 8. the tape and the modules
def test_backward_is_the_mode_2_launch(awm, dev):
    from awm_amd import ops
    n, n_out, L, S = 1000, 1300, 256, 64
    x = to_dev(Y.speech_rows(3, n, 21), dev).reshape(3, 1, n).requires_grad_(True)
    rate = to_dev(np.array([0.8, 1.25, 1.0]), dev).requires_grad_(True)
    g = to_dev(np.random.default_rng(55).standard_normal((3, 1, n_out)), dev)
    y, delta = ops.WsolaFn.apply(x, rate, n_out, L, S)
    assert tuple(y.shape) == (3, 1, n_out) and delta.dtype == torch.int32 and tuple(delta.shape) == (3, Y.frames(n_out, L)) and not delta.requires_grad
    y.backward(g)
    assert rate.grad is None, "the rate is a constant of the graph"
    dx = ops.wsola(g, rate.detach(), n, delta, adjoint=True, L=L, S=S)
    assert tuple(x.grad.shape) == (3, 1, n) and torch.equal(bits(x.grad), bits(dx)), "backward is the mode-2 launch, bit for bit"
    y0, d0 = ops.wsola(x.detach(), rate.detach(), n_out, L=L, S=S)
    assert torch.equal(bits(y0), bits(y.detach())) and torch.equal(d0, delta)
    y1, d1 = ops.wsola(x.detach(), rate.detach(), n_out, delta, L=L, S=S)
    assert torch.equal(bits(y1), bits(y0)) and d1 is not None
    gx, g64, dn = x.grad.cpu().numpy().reshape(3, n), g.cpu().numpy().reshape(3, n_out).astype(np.float64), delta.cpu().numpy()
    for r, rt in enumerate((0.8, 1.25, 1.0)):
        M = Y.matrix(rt, dn[r], n, n_out, L, S)
        _, bnd = Y.adjoint(g64[r], rt, dn[r], n, L, S)
        err = np.abs(gx[r] - M.T @ g64[r])
        print(f"rate {rt}: gradient against the dense matrix, worst err / bound {ratio(err, bnd):.4f}")
        assert (err <= bnd + 1e-12 * np.abs(M.T).dot(np.abs(g64[r]))).all() and np.abs(M).sum() > 10


@pytest.mark.parametrize("shape", [(5, 1, 2500), (2, 1300), (700,)])
def test_time_stretch_is_the_launch_with_its_draws(awm, dev, shape):
    from awm_amd import attacks, ops
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    n = shape[-1]
    x = to_dev(Y.speech_rows(rows, n, 61).reshape(shape), dev)
    att = awm.TimeStretch(rate=(0.8, 1.25), frame=256, search=64, seed=8)
    y = att(x, row0=4)
    want = Y.stretch_rates(8, 0, 4 + np.arange(rows), (0.8, 1.25))
    assert y.shape == x.shape and y.is_cuda and att.draw == 1 and not att.last_params.is_cuda
    assert np.array_equal(att.last_params.numpy(), want) and np.array_equal(attacks.row_stretch_rates(8, 0, 4 + np.arange(rows), (0.8, 1.25)), want)
    y0, d0 = ops.wsola(x.reshape(rows, n), to_dev(want, dev), L=256, S=64)
    assert torch.equal(bits(y.reshape(rows, n)), bits(y0)) and torch.equal(att.last_delta, d0)
    b = att(x, row0=4)
    assert att.draw == 2 and not torch.equal(b, y)
    assert torch.equal(bits(att.reset()(x, row0=4)), bits(y)) and torch.equal(bits(att.reset(1)(x, row0=4)), bits(b)), "reset rewinds"
    if rows > 2:
        whole = att.reset()(x)
        parts = torch.cat([att.reset()(x[:2]), att.reset()(x[2:], row0=2)])
        assert torch.equal(bits(whole), bits(parts)), "a batch cut into pieces draws what the whole batch does"


def test_pitch_shift_is_the_chain_of_the_two_launches(awm, dev):
    from awm_amd import ops
    n, rows = 2500, 4
    x = to_dev(Y.speech_rows(rows, n, 62).reshape(rows, 1, n), dev)
    att = awm.PitchShift(semitones=(-4, 4), frame=256, search=64, seed=9)
    y = att(x, row0=3)
    st_, beta, rate = Y.pitch_params(9, 0, 3 + np.arange(rows), (-4, 4))
    assert y.shape == x.shape and np.array_equal(att.last_params.numpy(), np.stack([st_, beta, rate], axis=1)) and att.draw == 1
    assert beta.min() < 1 < beta.max()
    for r in range(rows):
        m = max(n, int(np.ceil(float(beta[r]) * n)))
        z, delta = ops.wsola(x[r], to_dev(rate[r:r + 1], dev), m, L=256, S=64)
        prm = to_dev(np.array([[beta[r], 0, 0, 0, 0, min(1.0, 1.0 / float(beta[r]))]]), dev)
        want = ops.time_warp(z, prm)[:, :n]
        assert torch.equal(bits(y[r]), bits(want)), f"row {r}: the batch equals the row on its own, cut at its own m = {m}"
        assert torch.equal(att.last_delta[r, :delta.shape[1]], delta[0])
    whole = att.reset()(x)
    parts = torch.cat([att.reset()(x[:1]), att.reset()(x[1:], row0=1)])
    assert torch.equal(bits(whole), bits(parts)), "a batch cut into pieces draws what the whole batch does"
    assert torch.equal(bits(awm.PitchShift(semitones=0.0)(x)), bits(x)), "no shift: the identity, bit for bit"
    xg = x.clone().requires_grad_(True)
    att.reset()(xg).square().sum().backward()
    assert bool(torch.isfinite(xg.grad).all()) and bool((xg.grad != 0).any())


@pytest.mark.parametrize("L,S", Y.DIMS)
def test_cpu_path_agrees_on_integers(awm, dev, L, S):
    n = 1000
    x = np.concatenate([Y.integer_rows(n, 31 + L)] * 2)
    for rate in (0.8, 1.25):
        gpu, cpu = awm.TimeStretch(rate=rate, frame=L, search=S), awm.TimeStretch(rate=rate, frame=L, search=S)
        yg, yc = gpu(to_dev(x, dev)).cpu().numpy(), cpu(torch.from_numpy(x)).numpy()
        assert torch.equal(gpu.last_delta.cpu(), cpu.last_delta) and bool(cpu.last_delta.any()), "every score is exact: the same offsets"
        for r in range(len(x)):
            ref, bnd = Y.synth(x[r], rate, cpu.last_delta[r].numpy(), n, L, S)
            assert (np.abs(yg[r] - ref) <= bnd).all() and (np.abs(yc[r] - ref) <= bnd).all()


def test_train_step_through_the_stretch(awm, dev):
    """T = 2048: the shortest clip the step's loudness loss accepts"""
    G, D = reference_models(awm, dev)
    s = O.synthetic_clips(2, seed=41, T=2048).to(dev)
    msg = torch.tensor([3, 60001], device=dev)
    codec = torch.nn.Sequential(awm.TimeStretch(rate=(0.9, 1.1), seed=3), awm.PcmCodec(grad="straight_through"))
    G.train(); D.train()
    opt = torch.optim.Adam(list(G.parameters()) + list(D.parameters()), lr=1e-3)
    out = awm.train_step(G, D, opt, s, msg, codec=codec)
    assert codec[0].draw == 1 and tuple(codec[0].last_params.shape) == (2,) and tuple(codec[0].last_delta.shape) == (2, Y.frames(2048, 512))
    for k, v in out.items():
        if torch.is_tensor(v) and v.dim() == 0:
            assert bool(torch.isfinite(v)), f"loss {k}"
    assert bool(torch.isfinite(out["total"]))
    for k, p in G.named_parameters():
        assert bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), f"Generator {k}"


def test_evaluate_robustness_with_both_modules(awm, dev):
    ck = np.load(os.path.join(os.path.dirname(__file__), "golden", "detector_best_unprefixed.npz"))
    D = awm.Detector(16)
    D.load_state_dict({k: torch.from_numpy(ck[k]) for k in ck.files})
    torch.manual_seed(17)
    G = awm.Generator(16)
    G.to(dev); D.to(dev)
    batches = [O.synthetic_clips(2, seed=51, T=2048), O.synthetic_clips(2, seed=52, T=2048)]
    messages = [torch.tensor([3, 60001]), torch.tensor([77, 12345])]
    atk = {"stretch_1.05": awm.TimeStretch(rate=1.05), "stretch_1": awm.TimeStretch(rate=1.0), "pitch_+1": awm.PitchShift(semitones=1.0),
           "pitch_0": awm.PitchShift(semitones=0.0)}
    res = awm.evaluate_robustness(G, D, batches, atk, device=dev, messages=messages)
    print(res)
    assert list(res) == ["none"] + list(atk)
    keys = ["bit_accuracy", "clean_prob", "delta_rms", "watermarked_prob"]
    for name in ("stretch_1.05", "pitch_+1"):
        assert sorted(res[name]) == keys and all(np.isfinite(res[name][k]) for k in keys)
    assert atk["stretch_1.05"].draw == 2 and atk["pitch_+1"].draw == 2, "one call per batch"
    for k in keys:
        assert res["stretch_1"][k] == res["none"][k] and res["pitch_0"][k] == res["none"][k], "rate 1 and 0 semitones are the identity"


# ------------------------------------------------------------------------------------------ 9. refusals
def test_bad_arguments(awm, dev):
    from awm_amd import ops
    for args in Y.BAD_ARGS:
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm.lib.wm_wsola(*args)
    x, r = torch.zeros(3, 1000, device=dev), torch.ones(3, device=dev)
    K = Y.frames(1000, 512)
    d = torch.zeros(3, K, dtype=torch.int32, device=dev)
    for bx, br, kw in ((x, torch.ones(2, device=dev), {}), (x, torch.ones(3, 1, device=dev), {}), (x, r.double(), {}), (x.double(), r, {}),
                       (torch.zeros(3, 0, device=dev), r, {}), (torch.zeros(0, 100, device=dev), torch.ones(0, device=dev), {}),
                       (torch.zeros((), device=dev), r[:1], {}), (x, r, dict(n_out=0)), (x, r, dict(n_out=2 ** 30 + 1)), (x, r, dict(n_out=100.0)),
                       (x, r, dict(L=500)), (x, r, dict(L=32)), (x, r, dict(L=2048)), (x, r, dict(S=0)), (x, r, dict(S=257)), (x, r, dict(L=64, S=33)),
                       (x, r, dict(delta=d[:, :-1])), (x, r, dict(delta=d[:2])), (x, r, dict(delta=d.long())), (x, r, dict(delta=d.float())),
                       (x, r, dict(delta=d.reshape(-1))), (x, r, dict(adjoint=True)), (x, r, dict(delta=d, n_out=2000)),
                       (x, r, dict(delta=torch.zeros(3, Y.frames(2000, 512), dtype=torch.int32, device=dev), n_out=2000, adjoint=True))):
        with pytest.raises(ValueError):
            ops.wsola(bx, br, **kw)
    with pytest.raises(RuntimeError):
        ops.wsola(x.cpu(), r)
    with pytest.raises(RuntimeError):
        ops.wsola(x, r.cpu())
    with pytest.raises(RuntimeError):
        ops.wsola(x, r, delta=d.cpu())
    with pytest.raises(TypeError):
        ops.wsola(x, [1.0] * 3)
    y, dd = ops.wsola(x, r, n_out=2000, delta=torch.zeros(3, Y.frames(2000, 512), dtype=torch.int32, device=dev))
    assert tuple(y.shape) == (3, 2000) and tuple(ops.wsola(y, r, 1000, dd, adjoint=True).shape) == (3, 1000)
    torch.cuda.synchronize()
