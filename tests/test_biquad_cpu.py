"""Host side of the biquad / 16-bit PCM codec path (no GPU): the coefficient and warm-up helpers of dsp.py, the CPU twins of
perceptual_postprocess and encode_pcm16, save_audio's unchanged host path, and the adjoint formula the straight-through backward uses."""
import math
import wave

import numpy as np
import pytest
import torch
from scipy.signal import lfilter

import awm_amd
from awm_amd import ops
from biquad_yardstick import section


@pytest.mark.parametrize("rate,cutoff", [(16000, 7000), (44100, 7000), (48000, 7000), (48000, 500), (16000, 50)])
def test_coeffs_reproduce_lowpass_biquad(rate, cutoff):
    c = ops.biquad_lowpass_coeffs(rate, cutoff)
    b32, a32 = (v.astype(np.float32) for v in section(rate, cutoff))
    assert len(c) == 5 and all(isinstance(v, float) for v in c)
    assert c == (float(b32[0]), float(b32[1]), float(b32[2]), float(a32[1]), float(a32[2]))
    assert all(float(np.float32(v)) == v for v in c), "every value is a float32"
    assert ops.biquad_lowpass_coeffs(rate, cutoff) is c, "cached"
    # the impulse response through the CPU path IS lfilter with these coefficients (amplitude 0.25: the clamp stays out of it)
    imp = torch.zeros(1, 300)
    imp[0, 0] = 0.25
    got = awm_amd.lowpass_biquad(imp, rate, cutoff)
    want = lfilter(np.array(c[:3], dtype=np.float32), np.array((1.0,) + c[3:], dtype=np.float32), imp.numpy(), axis=-1)
    assert np.array_equal(got.numpy(), want.astype(np.float32))


def test_coeffs_reject_bad_arguments():
    for bad in ((0, 7000), (-16000, 7000), (16000, 0), (16000, -5), (16000, 8000), (16000, 9000), (float("nan"), 7000),
                (16000, float("inf")), ("16k", 7000), (True, 7000)):
        with pytest.raises(ValueError):
            ops.biquad_lowpass_coeffs(*bad)
    with pytest.raises(ValueError):
        ops.biquad_lowpass_coeffs(16000, 7000, Q=0)


def test_biquad_warm_values():
    for (rate, cutoff), want in (((16000, 7000), 100), ((48000, 7000), 44), ((48000, 500), 599), ((16000, 50), 1997)):
        c = ops.biquad_lowpass_coeffs(rate, cutoff)
        W = ops.biquad_warm(c)
        assert W == want, (rate, cutoff, W)
        r = math.sqrt(c[4])                                       # complex pole pair: radius sqrt(a2)
        assert r ** W <= 2.0 ** -40 < r ** (W - 1), "the smallest such W"
    assert ops.biquad_warm(ops.BIQUAD_IDENTITY) == 0
    assert ops.biquad_warm((1.0, 0.0, 0.0, -0.5, 0.0)) == 40      # one real pole at 0.5
    with pytest.raises(ValueError):
        ops.biquad_warm((1.0, 0.0, 0.0, -2.0, 1.0))               # double pole on the unit circle
    with pytest.raises(ValueError):
        ops.biquad_warm((1.0, 0.0, 0.0))


def test_biquad_plan_is_a_function_of_the_section_alone():
    awm_amd.lib.load()                                            # host-only query of the built library: no GPU needed
    assert ops.biquad_plan(ops.biquad_lowpass_coeffs(16000, 7000)) == (100, 32)
    assert ops.biquad_plan(ops.biquad_lowpass_coeffs(48000, 500)) == (599, 32)
    assert ops.biquad_plan(ops.biquad_lowpass_coeffs(16000, 50)) == (-1, 0)


def test_ops_biquad_has_no_cpu_path():
    with pytest.raises(ValueError):
        ops.biquad(torch.zeros(2, 100), ops.biquad_lowpass_coeffs(16000, 7000))


@pytest.mark.parametrize("shape", [(3, 1, 500), (2, 777), (1000,)])
def test_perceptual_postprocess_cpu_twin(shape):
    x = 0.6 * torch.randn(*shape, generator=torch.Generator().manual_seed(3))
    want = torch.round(awm_amd.lowpass_biquad(x, 16000, 7000) * 32767) / 32767
    got = awm_amd.perceptual_postprocess(x)
    assert got.shape == x.shape and got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(awm_amd.PcmCodec()(x), want)
    want48 = torch.round(awm_amd.lowpass_biquad(x, 48000, 500) * 32767) / 32767
    assert torch.equal(awm_amd.PcmCodec(500, 48000)(x), want48)
    assert not torch.equal(want, want48)
    codes = (got * 32767).round()
    assert torch.equal(codes / 32767, got) and float(codes.abs().max()) <= 32767, "values on the 16-bit grid"
    with pytest.raises(ValueError):
        awm_amd.perceptual_postprocess(x, grad="straight_through")          # needs the adjoint kernel
    with pytest.raises(ValueError):
        awm_amd.perceptual_postprocess(x, grad="ste")
    with pytest.raises(ValueError):
        awm_amd.PcmCodec(grad="ste")
    with pytest.raises(ValueError):
        awm_amd.PcmCodec(9000, 16000)


def test_encode_pcm16_cpu():
    x = 0.9 * torch.randn(2, 4001, generator=torch.Generator().manual_seed(4))
    got = awm_amd.encode_pcm16(x, 48000)
    assert got.dtype == torch.int16 and got.shape == (2, 4001)
    assert torch.equal(got, awm_amd.pcm16(awm_amd.lowpass_biquad(x, 48000, 7000)))
    assert torch.equal(awm_amd.encode_pcm16(x[0]), awm_amd.pcm16(awm_amd.lowpass_biquad(x[:1], 16000, 7000)))
    assert torch.equal(awm_amd.encode_pcm16(x, lowpass_hz=None), awm_amd.pcm16(x))
    with pytest.raises(ValueError):
        awm_amd.encode_pcm16(x.view(1, 2, 4001))


def test_save_audio_default_device_writes_the_same_bytes(tmp_path):
    x = 0.9 * torch.randn(2, 3000, generator=torch.Generator().manual_seed(5))
    for lowpass in (7000, None):
        want = awm_amd.pcm16(x if lowpass is None else awm_amd.lowpass_biquad(x, 16000, lowpass)).numpy()
        ref = str(tmp_path / "ref.wav")
        with wave.open(ref, "wb") as w:
            w.setnchannels(2); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes(np.ascontiguousarray(want.T).astype("<i2").tobytes())
        paths = [str(tmp_path / f"{k}.wav") for k in "abc"]
        awm_amd.save_audio(x, paths[0], 16000, lowpass_hz=lowpass)
        awm_amd.save_audio(x, paths[1], 16000, lowpass_hz=lowpass, device=None)
        awm_amd.save_audio(x, paths[2], 16000, lowpass_hz=lowpass, device="cpu")
        for p in paths:
            assert open(p, "rb").read() == open(ref, "rb").read(), (p, lowpass)


def test_step_functions_take_codec():
    import inspect
    from awm_amd import main14b_2, step
    for fn in (step.forward_losses, step.train_step, step.eval_forward, awm_amd.evaluate_batches):
        assert inspect.signature(fn).parameters["codec"].default is None, fn.__name__
    assert "codec" not in inspect.signature(main14b_2.forward_losses).parameters      # that family keeps its signature
    assert inspect.signature(awm_amd.save_audio).parameters["device"].default is None
    for name in ("perceptual_postprocess", "PcmCodec", "encode_pcm16"):
        assert name in awm_amd.__all__


def test_adjoint_is_flip_filter_flip():
    """the backward of the zero-state recursion y = F x is gx = F^T g = flip(F(flip(g))): autograd through an explicit recursion, float64"""
    n = 50
    c = ops.biquad_lowpass_coeffs(16000, 7000)
    b0, b1, b2, a1, a2 = c
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(n, dtype=torch.float64, generator=gen).requires_grad_()
    g = torch.randn(n, dtype=torch.float64, generator=gen)
    zero = torch.zeros((), dtype=torch.float64)
    ys = []
    for t in range(n):
        x1 = x[t - 1] if t >= 1 else zero
        x2 = x[t - 2] if t >= 2 else zero
        y1 = ys[t - 1] if t >= 1 else zero
        y2 = ys[t - 2] if t >= 2 else zero
        ys.append(b0 * x[t] + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2)
    y = torch.stack(ys)
    want_y = lfilter([b0, b1, b2], [1.0, a1, a2], x.detach().numpy())
    assert np.abs(y.detach().numpy() - want_y).max() <= 1e-12
    y.backward(g)
    adj = lfilter([b0, b1, b2], [1.0, a1, a2], g.numpy()[::-1])[::-1]
    assert np.abs(x.grad.numpy() - adj).max() <= 1e-12


def test_launcher_rejects_bad_arguments_without_a_gpu():
    """hipErrorInvalidValue (1) comes back before anything is launched, so these calls need no device"""
    c = ops.biquad_lowpass_coeffs(16000, 7000)
    x, o, m = 1 << 20, 1 << 22, 1 << 24                              # made-up, never dereferenced addresses
    for args in ((x, o, None, None, *c, 0, 1000, 100, 0, 1, 0, None),          # rows < 1
                 (x, o, None, None, *c, 2, 0, 100, 0, 1, 0, None),             # n < 1
                 (None, o, None, None, *c, 2, 1000, 100, 0, 1, 0, None),       # null x
                 (x, None, None, None, *c, 2, 1000, 100, 0, 1, 0, None),       # null out
                 (x, x, None, None, *c, 2, 1000, 100, 0, 1, 0, None),          # in place
                 (x, x + 7996, None, None, *c, 2, 1000, 100, 0, 1, 0, None),   # out overlaps the last float of x
                 (x, x + 4000, None, None, *c, 2, 1000, 100, 2, 1, 0, None),   # int16 out inside x
                 (x, o, x + 4, None, *c, 2, 1000, 100, 0, 1, 0, None),         # mask_out inside x
                 (x, o, None, None, *c, 2, 1000, 100, 3, 1, 0, None),          # unknown mode
                 (x, o, None, None, *c, 2, 1000, 100, 2, 0, 0, None),          # int16 without clamp
                 (x, o, m, None, *c, 2, 1000, 100, 0, 1, 1, None),             # mask_out with reverse
                 (x, o, None, None, *c, 2, 1000, 1025, 0, 1, 0, None),         # warm-up beyond the chunk kernel's limit
                 (x, o, None, None, *c, 2, 1000, -2, 0, 1, 0, None),
                 (x + 2, o, None, None, *c, 2, 1000, 100, 0, 1, 0, None)):     # x not on a 4-byte boundary
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm_amd.lib.wm_biquad(*args)
