"""The way back of the embed path, on the host: `resample_add` (delta at the model rate -> the recording's rate, added to every channel) through
its CPU twin, and `read_audio`.

The yardstick is `yardstick()` below (the text of tests/test_gpu_resample.py; no conftest.py may carry it): torchaudio's documented default
design evaluated in float64 numpy over ALL K = 2*width + P taps of every phase as a dense matrix product -- no compact table, no conv1d,
nothing from the package.  `design` is cached here: the table of 16000 -> 16001 has 16001 x 16014 entries.

Tolerance (derived, nothing tuned, no rtol): with (u64, bound) = yardstick(delta[:n_d], delta_freq, R, C=1) cut to N samples,
    |up - u64| <= bound                                     (the roundings of the float32 sums of the filter, see test_gpu_resample.py)
    |out[c] - (x[c] + u64)| <= bound + spacing(float32(|x[c] + u64|))      (the same error carried through ONE more float32 add)."""
import functools
import math
import wave

import numpy as np
import pytest
import torch

import awm_amd
from awm_amd import ops

LPW, ROLLOFF, U = 6, 0.99, 2.0 ** -24
RATES = [48000, 44100, 22050, 11025, 8000, 16001]


@functools.lru_cache(maxsize=1)
def design(orig, new):
    """(P, Q, width, K, dense float32 table (Q, K)) from the published formula, float64 rounded once to float32"""
    g = math.gcd(orig, new)
    P, Q = orig // g, new // g
    base = min(P, Q) * ROLLOFF
    width = int(math.ceil(LPW * P / base))
    K = 2 * width + P
    j = np.arange(K, dtype=np.float64)[None, :]
    i = np.arange(Q, dtype=np.float64)[:, None]
    t = np.clip(((j - width) / P - i / Q) * base, -LPW, LPW)
    pt = np.pi * t
    sinc = np.where(pt == 0, 1.0, np.sin(pt) / np.where(pt == 0, 1.0, pt))
    h = (base / P) * sinc * np.cos(pt / (2 * LPW)) ** 2
    return P, Q, width, K, h.astype(np.float32)


def yardstick(xmono, orig, new, C=1):
    """float64 resampling of the float64 mono signal `xmono` (N,) -> (y (L,), bound (L,))"""
    P, Q, width, K, h32 = design(orig, new)
    h = h32.astype(np.float64)
    N = xmono.shape[0]
    L = -((-Q * N) // P)
    periods = N // P + 1
    xpad = np.concatenate([np.zeros(width), np.asarray(xmono, dtype=np.float64), np.zeros(width + P)])
    frames = np.lib.stride_tricks.sliding_window_view(xpad, K)[::P][:periods]            # (periods, K): xpad[m*P + j]
    n = (h32 != 0).sum(axis=1) + C
    gamma = n * U / (1 - n * U)                                                              # (Q,)
    y, bound = np.empty((periods, Q)), np.empty((periods, Q))
    step = max(1, 4_000_000 // K)
    for a in range(0, periods, step):
        f = np.ascontiguousarray(frames[a:a + step])
        y[a:a + step] = f @ h.T
        bound[a:a + step] = (np.abs(f) @ np.abs(h).T) * gamma[None, :]
    y, bound = y.reshape(-1)[:L], bound.reshape(-1)[:L]
    return y, bound + np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)


def signal(kind, C, N, rate, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return 0.5 * torch.randn(C, N, generator=g)
    t = torch.arange(N, dtype=torch.float64) / rate                                          # recording-like: partials + a noise floor
    x = sum(a * torch.sin(2 * math.pi * f * t + p) for a, f, p in ((0.4, 220.0, 0.1), (0.2, 1730.0, 1.0), (0.1, 5200.0, 2.0)))
    return (x[None, :].repeat(C, 1) * torch.linspace(1.0, 0.6, C, dtype=torch.float64)[:, None]).float() + 0.01 * torch.randn(C, N, generator=g)


def assert_within(y, ref, bound, what):
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    assert y.shape == ref.shape, f"{what}: {y.shape} vs {ref.shape}"
    if y.size:
        err = np.abs(y - ref)
        worst = int(np.argmax(err - bound))
        print(f"{what}: max err {err.max():.3e}, max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound), f"{what}: sample {worst}: err {err[worst]:.3e} > bound {bound[worst]:.3e}"


def delta_for(n_d, seed, extra=0):
    return 0.01 * torch.randn(n_d + extra, generator=torch.Generator().manual_seed(seed))


def assert_sum_within(out, up, x, u64, bound, what):
    """the two bounds of the module docstring; out (C, N), up (1, N), x (C, N) tensors, u64 / bound (N,) float64"""
    assert tuple(up.shape) == (1, x.shape[1]) and tuple(out.shape) == tuple(x.shape)
    assert out.dtype == torch.float32 and up.dtype == torch.float32
    assert_within(up.numpy(), u64, bound, f"{what} up")
    for c in range(x.shape[0]):
        want = x[c].double().numpy() + u64
        assert_within(out[c].numpy(), want, bound + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64), f"{what} out[{c}]")


# ------------------------------------------------------------------------------------------ A1. the CPU twin against float64
@pytest.mark.parametrize("R", RATES)
def test_cpu_twin_vs_float64(R):
    for k, (C, N) in enumerate([(1, 1), (2, 2), (2, 7 * R // 100 + 3), (6, R + 4321)]):
        n_d = ops.resample_length(N, R, 16000)
        assert n_d == math.ceil(16000 * N / R)
        x = signal("recording", C, N, R, seed=10 * k + C)
        delta = delta_for(n_d, seed=R + k)
        out, up = awm_amd.resample_add(x, delta, R)
        u64, bound = yardstick(delta.double().numpy(), 16000, R, C=1)
        assert u64.shape[0] >= N
        assert_sum_within(out, up, x, u64[:N], bound[:N], f"16000->{R} C={C} N={N}")


# ------------------------------------------------------------------------------------------ A2. what lies behind n_d is not read
@pytest.mark.parametrize("R", [48000, 44100, 8000])
def test_tail_of_delta_is_ignored(R):
    C, N = 2, R // 10 + 7
    n_d = ops.resample_length(N, R, 16000)
    x = signal("recording", C, N, R, seed=5)
    delta = delta_for(n_d, seed=6, extra=500)
    delta[n_d:] = float("nan")
    out, up = awm_amd.resample_add(x, delta.view(1, 1, -1), R)                          # any shape: read flat
    assert not torch.isnan(out).any() and not torch.isnan(up).any()
    out_cut, up_cut = awm_amd.resample_add(x, delta[:n_d], R)
    assert torch.equal(up, up_cut) and torch.equal(out, out_cut)


# ------------------------------------------------------------------------------------------ A3. equal rates
@pytest.mark.parametrize("C", [1, 3])
def test_equal_rates_add_delta_itself(C):
    N = 1234
    x = signal("recording", C, N, 16000, seed=7)
    delta = delta_for(N, seed=8, extra=66)
    for rate in (16000, 44100):
        out, up = awm_amd.resample_add(x, delta, rate, rate)
        assert torch.equal(out, x + delta[:N]) and torch.equal(up, delta[:N].view(1, N))
        keep = delta.clone()
        up.add_(1.0)                                                                      # up is the caller's to write: never a view of delta
        assert torch.equal(delta, keep)
    out, up = awm_amd.resample_add(x[0], delta, 16000)                                    # (N,) is one channel
    assert torch.equal(out, x[:1] + delta[:N])


# ------------------------------------------------------------------------------------------ A4. arguments
def test_argument_errors():
    x = torch.zeros(2, 300)
    n_d = ops.resample_length(300, 48000, 16000)
    assert n_d == 100
    awm_amd.resample_add(x, torch.zeros(n_d), 48000)
    with pytest.raises(ValueError):
        awm_amd.resample_add(x, torch.zeros(n_d - 1), 48000)
    with pytest.raises(ValueError):
        awm_amd.resample_add(torch.zeros(1, 2, 300), torch.zeros(n_d), 48000)
    with pytest.raises(ValueError):
        awm_amd.resample_add(x, torch.zeros(n_d), 0)
    with pytest.raises(ValueError):
        awm_amd.resample_add(x, torch.zeros(n_d), 48000, 0)


# ------------------------------------------------------------------------------------------ A5. read_audio
def test_read_audio_keeps_channels_and_rate(tmp_path):
    rng = np.random.default_rng(3)
    N = 44100 // 5 + 9
    pcm = rng.integers(-30000, 30000, size=(N, 2)).astype("<i2")
    p = str(tmp_path / "stereo.wav")
    with wave.open(p, "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(44100); w.writeframes(pcm.tobytes())
    x, rate = awm_amd.read_audio(p)
    assert rate == 44100 and isinstance(rate, int)
    assert tuple(x.shape) == (2, N) and x.dtype == torch.float32
    assert np.array_equal(x.numpy(), pcm.T.astype(np.float32) / 32768.0)
