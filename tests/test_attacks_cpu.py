"""Host side of the channel distortions (no GPU): the Philox / Box-Muller restatement the kernel is tested against, the CPU path of
Distortion and Lowpass, argument errors of the modules and of the C ABI, and evaluate_robustness over stub models."""
import math

import numpy as np
import pytest
import torch
from scipy.signal import lfilter

import awm_amd
from awm_amd import attacks

import draw_yardstick


def words(text):
    return [int(w, 16) for w in text.split()]


@pytest.mark.parametrize("counter,key,want", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    """the known-answer vectors published with Random123 (kat_vectors, philox4x32 10 rounds): the package's restatement and the tests'
    one yardstick, each pinned to the publication"""
    for philox in (attacks.philox4x32_10, draw_yardstick.philox4x32_10):
        out = philox(words(counter), words(key))
        assert out.dtype == np.uint32 and out.shape == (4,)
        assert [int(v) for v in out] == words(want)


def test_philox_broadcasts_over_counters():
    q = np.arange(5, dtype=np.uint64)
    out = attacks.philox4x32_10((q, 0, 7, 3), (11, 12))
    assert out.shape == (4, 5)
    for i in range(5):
        assert np.array_equal(out[:, i], attacks.philox4x32_10((i, 0, 7, 3), (11, 12)))
    with pytest.raises(ValueError):
        attacks.philox4x32_10((0, 0, 0), (0, 0))


def test_normal_noise_moments():
    """five-sigma bounds at n = 2^20: the mean has sigma 1/sqrt(n) (4.9e-3), the variance sqrt(2/n) (6.9e-3), the share of |z| > 3 is
    p = erfc(3 / sqrt 2) = 0.0026998 with sigma sqrt(p (1 - p) / n) (2.6e-4)"""
    n = 2 ** 20
    z = attacks.normal_noise(seed=1234, draw=0, row=0, n=n)
    assert z.dtype == np.float64 and z.shape == (n,)
    tail = float((np.abs(z) > 3).mean())
    print(f"mean {z.mean():.3e} var {z.var():.6f} tail {tail:.7f} max {np.abs(z).max():.3f}")
    assert abs(z.mean()) < 4.9e-3
    assert abs(z.var() - 1) < 6.9e-3
    assert abs(tail - 0.0026998) < 2.6e-4
    assert np.abs(z).max() <= 5.77
    # a prefix of a longer row is the shorter row: the value of a sample depends on its own index only
    assert np.array_equal(attacks.normal_noise(1234, 0, 0, 1001), z[:1001])
    assert not np.array_equal(attacks.normal_noise(1234, 1, 0, 1001), z[:1001])
    assert not np.array_equal(attacks.normal_noise(1234, 0, 1, 1001), z[:1001])
    assert not np.array_equal(attacks.normal_noise(1235, 0, 0, 1001), z[:1001])
    assert not np.array_equal(attacks.normal_noise(1234 + 2 ** 32, 0, 0, 1001), z[:1001]), "the seed's high word is part of the key"


@pytest.mark.parametrize("shape", [(3, 1, 500), (2, 777), (1000,)])
def test_identity_settings_return_the_input(shape):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(1))
    d = awm_amd.Distortion(gain_db=0, snr_db=None)
    y = d(x)
    assert y.shape == x.shape and y.dtype == torch.float32 and torch.equal(y, x) and y.data_ptr() != x.data_ptr()
    rows = x.numel() // x.shape[-1]
    assert d.last_stat.shape == (rows, 4)
    assert torch.equal(d.last_stat[:, 0], torch.ones(rows)) and torch.equal(d.last_stat[:, 1], torch.zeros(rows))
    assert torch.isinf(d.last_stat[:, 3]).all()
    assert torch.equal(awm_amd.Distortion(gain_db=(0, 0), snr_db=(10, 20), p_noise=0.0)(x), x)


def test_achieved_snr_and_gain():
    """The noise of a row has power s^2 mean(z^2), and mean(z^2) over n samples scatters around 1 with sigma sqrt(2/n): at n = 16000 that
    is 4.34 * sqrt(2/n) = 0.049 dB, so 0.05 dB is about ONE sigma of what a correct implementation achieves (seed 7 below draws rows
    0.14 dB off).  The bound is therefore asserted (a) as it stands on the two rows of (seed 5, draw 0), whose noise is 0.005 and 0.042 dB
    off, and (b) on every row of another seed once the realised mean(z^2) is taken out, where what is left is rounding: 1e-3 dB."""
    n = 16000
    x = 0.1 * torch.randn(4, 1, n, generator=torch.Generator().manual_seed(2))

    def achieved(d, x):
        y = d(x)
        st = d.last_stat.double()
        gx = st[:, 0, None, None] * x.double()
        return st, 10 * torch.log10(gx.pow(2).mean(dim=2) / (y.double() - gx).pow(2).mean(dim=2)).reshape(-1)

    st, snr = achieved(awm_amd.Distortion(gain_db=(-6, 6), snr_db=(20, 40), seed=5), x[:2])
    print("seed 5: achieved", snr.tolist(), "drawn", st[:, 3].tolist())
    assert (snr - st[:, 3]).abs().max() < 0.05
    st, snr = achieved(awm_amd.Distortion(gain_db=(-6, 6), snr_db=(20, 40), seed=7), x)
    z2 = torch.tensor([float((attacks.normal_noise(7, 0, r, n) ** 2).mean()) for r in range(4)], dtype=torch.float64)
    print("seed 7: achieved", snr.tolist(), "drawn", st[:, 3].tolist(), "mean z^2", z2.tolist())
    assert (snr + 10 * torch.log10(z2) - st[:, 3]).abs().max() < 1e-3
    assert ((st[:, 3] >= 20) & (st[:, 3] <= 40)).all()
    gain_db = 20 * torch.log10(st[:, 0])
    assert ((gain_db >= -6) & (gain_db <= 6)).all() and gain_db.std() > 0.1, "one gain per row"
    assert torch.allclose(st[:, 2], x.double().pow(2).mean(dim=2).reshape(-1), rtol=1e-6)
    assert torch.allclose(st[:, 1], st[:, 0] * st[:, 2].sqrt() * 10 ** (-st[:, 3] / 20), rtol=1e-6)
    # fixed values
    f = awm_amd.Distortion(gain_db=-3, snr_db=25)
    f(x)
    assert torch.allclose(f.last_stat[:, 0], torch.full((4,), 10 ** (-3 / 20)), rtol=1e-6)
    assert torch.equal(f.last_stat[:, 3], torch.full((4,), 25.0))


def test_draw_counter_and_reset():
    x = torch.randn(2, 1, 300, generator=torch.Generator().manual_seed(3))
    d = awm_amd.Distortion(seed=5)
    assert d.draw == 0
    a, b = d(x), d(x)
    assert d.draw == 2 and not torch.equal(a, b), "every call draws fresh noise"
    assert torch.equal(d.reset()(x), a) and torch.equal(d(x), b), "reset rewinds; the same (seed, draw) repeats"
    assert torch.equal(d.reset(1)(x), b)
    assert torch.equal(awm_amd.Distortion(seed=5)(x), a)
    assert not torch.equal(awm_amd.Distortion(seed=6)(x), a)
    # row0 numbers the rows: the second row alone, as row 1, is the second row of the batch
    assert torch.equal(d.reset()(x[1:], row0=1), a[1:])
    assert not torch.equal(d.reset()(x[1:]), a[1:])
    # p_noise = 0.5: the rows that get noise are the rows the coin names
    c = awm_amd.Distortion(gain_db=0, snr_db=10, p_noise=0.5, seed=0)
    big = torch.randn(64, 50, generator=torch.Generator().manual_seed(4))
    y = c(big)
    _, _, noisy = attacks.row_parameters(0, 0, np.arange(64), c.bounds)
    assert 16 < noisy.sum() < 48
    assert np.array_equal(((y - big).abs().amax(dim=1) > 0).numpy(), noisy)
    assert np.array_equal(torch.isfinite(c.last_stat[:, 3]).numpy(), noisy)


def test_module_argument_errors():
    D = awm_amd.Distortion
    for kw in (dict(gain_db=(6, -6)), dict(snr_db=(40, 20)), dict(gain_db=(1, 2, 3)), dict(gain_db=float("nan")),
               dict(snr_db=(0, float("inf"))), dict(gain_db="loud"), dict(p_noise=1.5), dict(p_noise=-0.1), dict(p_noise=None),
               dict(noise_grad="ste"), dict(seed=1.5), dict(gain_db=True)):
        with pytest.raises(ValueError):
            D(**kw)
    d = D()
    for bad in (torch.zeros(2, 2, 2, 2), torch.zeros(0), torch.zeros(2, 0)):
        with pytest.raises(ValueError):
            d(bad)
    with pytest.raises(TypeError):
        d([0.0, 1.0])
    assert d.draw == 0, "a refused call draws nothing"
    for bad in (-1, 2 ** 32, 1.0):
        with pytest.raises(ValueError):
            d(torch.zeros(2, 8), row0=bad)
        with pytest.raises(ValueError):
            d.reset(bad)
    assert "noise_grad='through'" in repr(d)
    with pytest.raises(ValueError):
        awm_amd.Lowpass(9000, 16000)
    with pytest.raises(ValueError):
        awm_amd.Lowpass(4000)(torch.zeros(1, 1, 1, 8))
    for name in ("attacks", "Distortion", "Lowpass", "evaluate_robustness"):
        assert name in awm_amd.__all__


def test_lowpass_cpu_is_the_section_without_clamp():
    x = 2.0 * torch.randn(2, 1, 400, generator=torch.Generator().manual_seed(5))
    c = awm_amd.ops.biquad_lowpass_coeffs(16000, 3000)
    want = lfilter(np.array(c[:3], dtype=np.float32), np.array((1.0,) + c[3:], dtype=np.float32), x.numpy(), axis=-1).astype(np.float32)
    got = awm_amd.Lowpass(3000)(x)
    assert got.shape == x.shape and np.array_equal(got.numpy(), want)
    assert float(got.abs().max()) > 1.0, "no clamp"


def test_launcher_rejects_bad_arguments_without_a_gpu():
    """hipErrorInvalidValue (1) comes back before anything is launched, so these calls need no device"""
    x, y, st, sc = 1 << 20, 1 << 22, 1 << 24, 1 << 26                # made-up, never dereferenced addresses
    b = (-6.0, 6.0, 20.0, 40.0, 1.0)
    nan, inf = float("nan"), float("inf")
    for args in ((x, y, st, sc, 0, 1000, 0, 0, 0, *b, None),                       # rows < 1
                 (x, y, st, sc, 2, 0, 0, 0, 0, *b, None),                          # n < 1
                 (x, y, st, sc, 1, (1 << 34) + 1, 0, 0, 0, *b, None),              # n above 2^34
                 (None, y, st, sc, 2, 1000, 0, 0, 0, *b, None),                    # null pointers
                 (x, None, st, sc, 2, 1000, 0, 0, 0, *b, None),
                 (x, y, None, sc, 2, 1000, 0, 0, 0, *b, None),
                 (x, y, st, None, 2, 1000, 0, 0, 0, *b, None),
                 (x, x, st, sc, 2, 1000, 0, 0, 0, *b, None),                       # in place
                 (x, x + 7996, st, sc, 2, 1000, 0, 0, 0, *b, None),                # y overlaps the last float of x
                 (x + 2, y, st, sc, 2, 1000, 0, 0, 0, *b, None),                   # x not on a 4-byte boundary
                 (x, y, st, sc, 2, 1000, -1, 0, 0, *b, None),                      # row0 < 0
                 (x, y, st, sc, 2, 1000, (1 << 32) - 1, 0, 0, *b, None),           # row0 + rows > 2^32
                 (x, y, st, sc, 2, 1000, 0, 0, -1, *b, None),                      # draw out of range
                 (x, y, st, sc, 2, 1000, 0, 0, 1 << 32, *b, None),
                 (x, y, st, sc, 2, 1000, 0, 0, 0, -6.0, 6.0, 20.0, 40.0, 1.5, None),   # p_noise outside [0, 1]
                 (x, y, st, sc, 2, 1000, 0, 0, 0, -6.0, 6.0, 20.0, 40.0, -0.5, None),
                 (x, y, st, sc, 2, 1000, 0, 0, 0, -6.0, 6.0, 20.0, 40.0, nan, None),
                 (x, y, st, sc, 2, 1000, 0, 0, 0, 6.0, -6.0, 20.0, 40.0, 1.0, None),   # lo > hi
                 (x, y, st, sc, 2, 1000, 0, 0, 0, -6.0, 6.0, 40.0, 20.0, 1.0, None),
                 (x, y, st, sc, 2, 1000, 0, 0, 0, -inf, 6.0, 20.0, 40.0, 1.0, None),   # non-finite bounds
                 (x, y, st, sc, 2, 1000, 0, 0, 0, -6.0, 6.0, 20.0, inf, 1.0, None),
                 (x, y, st, sc, 2, 1000, 0, 0, 0, nan, nan, 20.0, 40.0, 1.0, None)):
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm_amd.lib.wm_distort(*args)
    dy, dx = 1 << 27, 1 << 28
    for args in ((dy, x, st, dx, sc, 0, 1000, 0, 0, 0, 1, None),                   # rows < 1
                 (dy, x, st, dx, sc, 2, 0, 0, 0, 0, 1, None),                      # n < 1
                 (None, x, st, dx, sc, 2, 1000, 0, 0, 0, 1, None),                 # null pointers
                 (dy, None, st, dx, sc, 2, 1000, 0, 0, 0, 1, None),
                 (dy, x, None, dx, sc, 2, 1000, 0, 0, 0, 1, None),
                 (dy, x, st, None, sc, 2, 1000, 0, 0, 0, 1, None),
                 (dy, x, st, dx, None, 2, 1000, 0, 0, 0, 0, None),
                 (dy, x, st, dy, sc, 2, 1000, 0, 0, 0, 1, None),                   # dx is dy
                 (dy, x, st, x + 4000, sc, 2, 1000, 0, 0, 0, 0, None),             # dx inside x
                 (dy, x, st, dx, sc, 2, 1000, 0, 0, 1 << 32, 1, None)):            # draw out of range
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm_amd.lib.wm_distort_bwd(*args)


def test_distort_plan_is_a_function_of_the_shape():
    import ctypes
    need = ctypes.c_longlong(0)
    for rows, n, want in ((1, 1, 2), (512, 16000, 1024), (3, 16384, 6), (3, 16385, 9), (1, 10 ** 7, 612)):
        awm_amd.lib.wm_distort_plan(rows, n, ctypes.addressof(need), None)
        assert need.value == want, (rows, n, need.value)
    with pytest.raises(RuntimeError, match="hipError 1$"):
        awm_amd.lib.wm_distort_plan(0, 5, ctypes.addressof(need), None)


class StubGenerator(torch.nn.Module):
    def forward(self, s, message):
        self.calls = getattr(self, "calls", 0) + 1
        return 0.01 * torch.sign(s) * (1 + (message % 3)).view(-1, 1, 1).float()


class StubDetector(torch.nn.Module):
    """logit 0 rises with the clip's level, logit 1 + b says bit b is set where the clip's mean is positive"""
    def __init__(self, bits):
        super().__init__()
        self.bits, self.seen = bits, []

    def forward(self, x):
        self.seen.append(x.clone())
        R = 5
        level = x.abs().mean(dim=2)                                              # (2B, 1)
        det = (level * 4 - 1).expand(-1, R)
        bit = (x.mean(dim=2) * 100).expand(-1, R)
        return torch.cat([det.unsqueeze(2), bit.unsqueeze(2).expand(-1, -1, self.bits)], dim=2)


def test_evaluate_robustness_on_stubs(monkeypatch):
    """the delta post-processing is a HIP kernel with no CPU path: the identity stands in for it here"""
    monkeypatch.setattr(attacks, "postprocess", lambda d: d)
    bits = 4
    gen = torch.Generator().manual_seed(6)
    batches = [0.3 * torch.randn(3, 1, 64, generator=gen).abs(), 0.3 * torch.randn(2, 1, 64, generator=gen).abs()]   # ragged last batch
    messages = [torch.tensor([15, 15, 15]), torch.tensor([15, 0])]
    G, D = StubGenerator(), StubDetector(bits)
    G.train(); D.train()
    atk = {"half": awm_amd.Distortion(gain_db=20 * math.log10(0.5), snr_db=None), "flip": awm_amd.Distortion(0, None)}
    res = awm_amd.evaluate_robustness(G, D, batches, atk, device="cpu", message_bits=bits, messages=messages)
    assert list(res) == ["none", "half", "flip"]
    assert all(sorted(v) == ["bit_accuracy", "clean_prob", "delta_rms", "watermarked_prob"] for v in res.values())
    assert not G.training and not D.training and G.calls == 2, "eval mode; one Generator call per batch"
    assert len(D.seen) == 6 and [t.shape[0] for t in D.seen] == [6, 6, 6, 4, 4, 4], "one Detector call per attack, on the concatenation"
    # the attack reaches both halves: watermarked and clean
    for k, s in ((0, batches[0]), (3, batches[1])):
        none, half = D.seen[k], D.seen[k + 1]
        B = s.shape[0]
        assert torch.equal(none[B:], s) and not torch.equal(none[:B], s)
        assert torch.allclose(half, 0.5 * none, rtol=1e-6, atol=0) and not torch.equal(half, none)
        assert torch.equal(D.seen[k + 2], none)
    assert res["flip"] == res["none"]
    # pooled over the five clips, not averaged per batch
    per_clip = torch.cat([torch.sigmoid(D.seen[k][:B].abs().mean(dim=2) * 4 - 1).reshape(-1) for k, B in ((0, 3), (3, 2))])
    assert res["none"]["watermarked_prob"] == pytest.approx(float(per_clip.double().mean()), rel=1e-6)
    assert res["none"]["watermarked_prob"] > res["half"]["watermarked_prob"] > 0
    assert res["none"]["clean_prob"] > res["half"]["clean_prob"]
    assert res["none"]["bit_accuracy"] == pytest.approx(4 / 5), "message 0 on an all-positive clip decodes wrong; 4 of 5 clips right"
    rms = torch.cat([0.01 * (1 + (m % 3)).float() for m in messages])
    assert res["none"]["delta_rms"] == pytest.approx(float(rms.double().mean()), rel=1e-6)
    assert res["half"]["delta_rms"] == res["none"]["delta_rms"], "delta itself is not attacked"
    with pytest.raises(ValueError):
        awm_amd.evaluate_robustness(G, D, batches, {"none": atk["half"]}, device="cpu")
    empty = awm_amd.evaluate_robustness(G, D, [], atk, device="cpu")
    assert math.isnan(empty["half"]["clean_prob"])
