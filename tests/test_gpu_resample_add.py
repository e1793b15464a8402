"""The way back of the embed path on the GPU: wm_resample_add (csrc/resample.hip) takes delta from the model rate up to the recording's rate
and adds it to every channel of the untouched recording in one launch; `ops.resample_add`, `resample_add`, and the `native_rate=True`
keyword of embed_waveform / generate_watermarked_audio on top of it.

The yardstick is `yardstick()` of tests/resample_yardstick.py, float64 numpy with nothing from the package; the two derived bounds
(`up` against u64, `out[c]` through one more float32 add) stand in that module's docstring under "resample_add".
Beyond that the kernel is held to bit identity: up is ops.resample of the same samples, out is one torch add.  Model outputs downstream
of it: FWD_TOL, as everywhere in this suite."""
import math
import wave

import numpy as np
import pytest
import torch

from gpu_support import awm, dev  # noqa: F401
from gpu_support import check, reference_models, same
from resample_yardstick import LPW, ROLLOFF, signal, yardstick
from yardstick_common import assert_within

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4

RATES = [48000, 44100, 32000, 22050, 11025, 8000]


def pq(delta_rate, rate):
    g = math.gcd(delta_rate, rate)
    return delta_rate // g, rate // g


def n_delta(N, rate):
    return -((-16000 * N) // rate)


_REF = {}


def reference(rate, N, extra=0):
    """(delta (n_d + extra,) CPU, u64 (N,), bound (N,)) of one (rate, N): computed once, shared by every test and channel count, never
    written to.  The `extra` samples behind n_d are NaN: nothing may read them."""
    key = (rate, N, extra)
    if key not in _REF:
        n_d = n_delta(N, rate)
        delta = 0.01 * torch.randn(n_d + extra, generator=torch.Generator().manual_seed(rate + N))
        delta[n_d:] = float("nan")
        u64, bound = yardstick(delta[:n_d].double().numpy(), 16000, rate, C=1)
        assert u64.shape[0] >= N
        _REF[key] = (delta, u64[:N], bound[:N])
    return _REF[key]


def lengths(rate, tile):
    P, Q = pq(16000, rate)
    return [N for N in (1, 2, Q - 1, Q, 7 * Q + 3, tile * Q - 1, 3 * tile * Q + 5, rate + 4321) if N > 0]


def assert_sum_within(out, up, x, u64, bound, what):
    """the two bounds of the module docstring; out (C, N), up (1, N), x (C, N) CPU tensors, u64 / bound (N,) float64"""
    assert tuple(up.shape) == (1, x.shape[1]) and tuple(out.shape) == tuple(x.shape)
    assert_within(up.numpy(), u64, bound, f"{what} up")
    for c in range(x.shape[0]):
        want = x[c].double().numpy() + u64
        assert_within(out[c].numpy(), want, bound + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64), f"{what} out[{c}]")


def assert_bit_identity(ops, x, delta, rate, out, up):
    """B2: up is the existing resampler's result for the same samples, out is one torch add, with or without up, in place or not"""
    C, N = x.shape
    n_d = n_delta(N, rate)
    want_up = ops.resample(delta[:n_d].view(1, -1), 16000, rate)[:, :N]
    assert torch.equal(up, want_up), "up differs from ops.resample of the same samples"
    for c in range(C):
        assert torch.equal(out[c], x[c] + up[0]), f"out[{c}] is not x[{c}] + up"
    out2, none = ops.resample_add(x, delta, rate, want_up=False)
    assert none is None and torch.equal(out2, out)
    xc = x.clone()
    out3, up3 = ops.resample_add(xc, delta, rate, out=xc)
    assert out3 is xc and torch.equal(xc, out) and torch.equal(up3, up)


# ------------------------------------------------------------------------------------------ B1 / B2. the kernel against float64, and bit for bit
@pytest.mark.parametrize("C", [1, 2, 6])
@pytest.mark.parametrize("rate", RATES)
def test_kernel_vs_float64(awm, dev, rate, C):
    from awm_amd import ops
    tile = ops.resample_tile_periods(16000, rate)
    assert tile > 0 and tile % 4 == 0
    for k, N in enumerate(lengths(rate, tile)):
        delta, u64, bound = reference(rate, N, extra=3)
        x = signal("recording", C, N, rate, seed=100 * C + k)
        out, up = ops.resample_add(x.to(dev), delta.to(dev), rate)
        assert out.is_cuda and up.is_cuda and out.dtype == torch.float32 and up.dtype == torch.float32
        assert_sum_within(out.cpu(), up.cpu(), x, u64, bound, f"16000->{rate} C={C} N={N}")


@pytest.mark.parametrize("C", [1, 2, 6])
@pytest.mark.parametrize("rate", RATES)
def test_bit_identity(awm, dev, rate, C):
    from awm_amd import ops
    tile = ops.resample_tile_periods(16000, rate)
    for k, N in enumerate(lengths(rate, tile)):
        delta = reference(rate, N, extra=3)[0].to(dev)
        x = signal("recording", C, N, rate, seed=200 * C + k).to(dev)
        out, up = awm.resample_add(x, delta, rate)                                     # the public entry: a CUDA tensor goes to the kernel
        assert_bit_identity(ops, x, delta, rate, out, up)


# ------------------------------------------------------------------------------------------ B3. written once, nowhere else
def launch_raw(awm, dev, rate, C, N, x_off, d_off, out_off, up_off, guard=64):
    """wm_resample_add on hand-made buffers: x and delta start `x_off` / `d_off` floats into their allocations, out and up are slices
    `out_off` / `up_off` floats into NaN-filled buffers with at least `guard` floats of NaN on either side"""
    from awm_amd import ops
    tab = ops.resample_table(16000, rate)
    taps, first = tab["taps"].to(dev), tab["first"].to(dev)
    delta, u64, bound = reference(rate, N, extra=37)
    n_d = n_delta(N, rate)
    x = signal("recording", C, N, rate, seed=300 + C)
    xbuf = torch.full((x_off + C * N + guard,), float("nan"), device=dev)
    xv = xbuf[x_off:x_off + C * N].view(C, N)
    xv.copy_(x)
    dbuf = torch.full((d_off + delta.numel() + guard,), float("nan"), device=dev)
    dv = dbuf[d_off:d_off + delta.numel()]
    dv.copy_(delta)                                                                     # its tail behind n_d is NaN already
    obuf = torch.full((out_off + C * N + guard,), float("nan"), device=dev)
    ubuf = torch.full((up_off + N + guard,), float("nan"), device=dev)
    ov, uv = obuf[out_off:out_off + C * N], ubuf[up_off:up_off + N]
    awm.lib.wm_resample_add(dv.data_ptr(), taps.data_ptr(), first.data_ptr(), xv.data_ptr(), ov.data_ptr(), uv.data_ptr(), C, N, n_d,
                            tab["P"], tab["Q"], tab["width"], tab["W"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for name, buf, off, n in (("out", obuf, out_off, C * N), ("up", ubuf, up_off, N)):
        b = buf.cpu()
        assert not torch.isnan(b[off:off + n]).any(), f"{name}: samples left unwritten (or NaN read from behind n_d)"
        assert torch.isnan(b[:off]).all() and torch.isnan(b[off + n:]).all(), f"{name}: written outside its {n} samples"
    assert_sum_within(ov.view(C, N).cpu(), uv.view(1, N).cpu(), x, u64, bound, f"raw 16000->{rate} C={C} N={N}")
    assert torch.equal(uv.view(1, N), ops.resample(dv[:n_d].view(1, -1), 16000, rate)[:, :N])
    assert torch.equal(ov.view(C, N), xv + uv)


@pytest.mark.parametrize("rate", [48000, 44100, 8000])
def test_written_once_nowhere_else(awm, dev, rate):
    from awm_amd import ops
    tile = ops.resample_tile_periods(16000, rate)
    P, Q = pq(16000, rate)
    odd = 2 * tile * Q + 2 * Q + 1                                                      # tile % 4 == 0: odd, the second row is off the 16-byte grid
    assert odd % 2 == 1
    launch_raw(awm, dev, rate, 2, odd, x_off=1, d_off=1, out_off=67, up_off=65)        # nothing aligned: 4-byte accesses
    launch_raw(awm, dev, rate, 2, odd, x_off=0, d_off=0, out_off=64, up_off=64)        # aligned pointers, odd N: still 4-byte rows
    quad = (odd + 3) // 4 * 4
    assert quad % 4 == 0
    launch_raw(awm, dev, rate, 2, quad, x_off=0, d_off=1, out_off=64, up_off=128)      # 16-byte rows, delta off the grid
    launch_raw(awm, dev, rate, 3, quad, x_off=4, d_off=4, out_off=68, up_off=64)       # 16-byte rows everywhere
    launch_raw(awm, dev, rate, 2, quad, x_off=0, d_off=0, out_off=64, up_off=65)       # one misaligned pointer sends all rows the 4-byte way


# ------------------------------------------------------------------------------------------ B4. a table that does not fit LDS
@pytest.mark.parametrize("C", [1, 2])
def test_table_that_does_not_fit_lds(awm, dev, C):
    """16000 -> 16001 has 16 001 phases: the one-thread-per-sample kernel, table through the cache"""
    from awm_amd import ops
    assert ops.resample_tile_periods(16000, 16001) == 0
    for N in (1, 16001, 40003):
        delta, u64, bound = reference(16001, N, extra=3)
        x = signal("recording", C, N, 16001, seed=40 + C)
        out, up = ops.resample_add(x.to(dev), delta.to(dev), 16001)
        assert_sum_within(out.cpu(), up.cpu(), x, u64, bound, f"16000->16001 C={C} N={N}")
        assert_bit_identity(ops, x.to(dev), delta.to(dev), 16001, out, up)


# ------------------------------------------------------------------------------------------ B5. minutes
@pytest.mark.parametrize("rate,C,N", [(48000, 2, 48000 * 200), (44100, 1, 44100 * 190 + 3)])
def test_kernel_vs_float64_minutes(awm, dev, rate, C, N):
    """several minutes: every workgroup walks more than one tile, channel rows are megabytes apart"""
    from awm_amd import ops
    delta, u64, bound = reference(rate, N)
    x = signal("noise", C, N, rate, seed=7 + C)
    out, up = ops.resample_add(x.to(dev), delta.to(dev), rate)
    assert_sum_within(out.cpu(), up.cpu(), x, u64, bound, f"16000->{rate} C={C} {N} samples")


# ------------------------------------------------------------------------------------------ B6. shift, bit for bit
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("rate", RATES + [16001])
def test_shift_is_bit_exact(awm, dev, rate, C):
    """the additions of a sample depend on its phase only: delta delayed by d input periods (P samples) and x by d*Q samples give up (and out)
    delayed by d*Q samples, identically, wherever the sample then falls in a tile or a workgroup"""
    from awm_amd import ops
    P, Q = pq(16000, rate)
    width = ops.resample_table(16000, rate)["width"]
    assert width == int(math.ceil(LPW * P / (min(P, Q) * ROLLOFF)))
    tile = ops.resample_tile_periods(16000, rate)
    N = (3 * tile + 40) * Q + 11 if tile else 6 * Q + 11
    n_d = n_delta(N, rate)
    delta = (0.01 * torch.randn(n_d, generator=torch.Generator().manual_seed(61))).to(dev)
    x = signal("noise", C, N, rate, seed=60 + C).to(dev)
    out, up = ops.resample_add(x, delta, rate)
    edge = (math.ceil(width / P) + 1) * Q
    a, b = edge, N - edge
    assert b - a > Q
    for d in [1, 7] + ([tile, tile + 3] if tile else []):
        ds = torch.cat([torch.zeros(d * P, device=dev), delta])
        xs = torch.cat([torch.zeros(C, d * Q, device=dev), x], dim=1)
        assert n_delta(N + d * Q, rate) == n_d + d * P
        outs, ups = ops.resample_add(xs, ds, rate)
        assert torch.equal(ups[0, a + d * Q:b + d * Q], up[0, a:b]), f"16000->{rate}: delay of {d} periods changes the samples of up"
        assert torch.equal(outs[:, a + d * Q:b + d * Q], out[:, a:b]), f"16000->{rate}: delay of {d} periods changes the samples of out"


# ------------------------------------------------------------------------------------------ B7. equal rates, and the arguments
def test_equal_rates(awm, dev):
    from awm_amd import ops
    for N in (1, 4099, 40000):
        x = signal("recording", 3, N, 16000, seed=70).to(dev)
        delta = torch.randn(N + 5, device=dev) * 0.01
        delta[N:] = float("nan")
        out, up = ops.resample_add(x, delta, 16000)
        assert torch.equal(out, x + delta[:N]) and torch.equal(up, delta[:N].view(1, N))
        out, up = ops.resample_add(x, delta, 44100, 44100)
        assert torch.equal(out, x + delta[:N])


def test_arguments(awm, dev):
    from awm_amd import ops
    x = torch.zeros(2, 300, device=dev)
    d = torch.zeros(100, device=dev)
    out, up = ops.resample_add(x, d, 48000)
    assert tuple(out.shape) == (2, 300) and tuple(up.shape) == (1, 300)
    out, up = ops.resample_add(x[0], d, 48000)                                        # (N,) is one channel
    assert tuple(out.shape) == (1, 300)
    x1 = torch.ones(300, device=dev)
    out, up = ops.resample_add(x1, d + 1, 48000, out=x1)                                # in place on a (N,) tensor: lands in it
    assert tuple(out.shape) == (1, 300) and out.data_ptr() == x1.data_ptr() and torch.equal(x1, 1 + up[0]) and bool((up != 0).all())
    out, up = ops.resample_add(torch.zeros(2, 0, device=dev), d, 48000)                # N == 0: no launch
    assert tuple(out.shape) == (2, 0) and tuple(up.shape) == (1, 0)
    with pytest.raises(RuntimeError):
        ops.resample_add(torch.zeros(2, 300), torch.zeros(100), 48000)                  # a CPU tensor has no business in ops
    with pytest.raises(ValueError):
        ops.resample_add(x, d[:99], 48000)
    with pytest.raises(ValueError):
        ops.resample_add(torch.zeros(1, 2, 300, device=dev), d, 48000)
    with pytest.raises(ValueError):
        ops.resample_add(x, d, 0)
    with pytest.raises(ValueError):
        ops.resample_add(x, d, 48000, out=torch.zeros(2, 299, device=dev))
    tab = ops.resample_table(16000, 48000)
    taps, first = tab["taps"].to(dev), tab["first"].to(dev)
    out = torch.zeros(2, 300, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    args = (tab["P"], tab["Q"], tab["width"], tab["W"], s)
    for bad in ((d.data_ptr(), taps.data_ptr(), first.data_ptr(), x.data_ptr(), out.data_ptr(), None, 0, 300, 100) + args,     # C = 0
                (d.data_ptr(), taps.data_ptr(), first.data_ptr(), x.data_ptr(), out.data_ptr(), None, 2, -1, 100) + args,      # N < 0
                (d.data_ptr(), taps.data_ptr(), first.data_ptr(), x.data_ptr(), out.data_ptr(), None, 2, 300, -1) + args,      # Nd < 0
                (d.data_ptr(), taps.data_ptr(), first.data_ptr(), None, out.data_ptr(), None, 2, 300, 100) + args,             # x NULL
                (d.data_ptr(), taps.data_ptr(), first.data_ptr(), x.data_ptr(), out.data_ptr(), None, 65537, 300, 100) + args,  # C > 65536
                (d.data_ptr(), taps.data_ptr(), first.data_ptr(), x.data_ptr(), x.data_ptr(), None, 2, 300, 100, 1, 3, 7, 16, s)):  # W > K
        with pytest.raises(RuntimeError, match="hipError 1"):
            awm.lib.wm_resample_add(*bad)


# ------------------------------------------------------------------------------------------ B8 - B10. the file-level entry points
@pytest.fixture(scope="module")
def models(awm, dev):
    return reference_models(awm, dev)


def test_embed_waveform_native_rate(awm, dev, models):
    G, _ = models
    N = 48000 * 2 + 15000
    x48 = signal("recording", 2, N, 48000, seed=83)
    keep = x48.clone()
    msgs = torch.tensor([11, 22222, 65535])
    wm, delta, orig = awm.embed_waveform(x48, G, device=dev, messages=msgs, orig_freq=48000, native_rate=True)
    assert tuple(wm.shape) == (2, N) and tuple(delta.shape) == (1, N) and tuple(orig.shape) == (2, N)
    assert not wm.is_cuda and not delta.is_cuda and not orig.is_cuda
    assert torch.equal(orig, keep) and torch.equal(x48, keep)
    assert torch.equal(wm, orig + delta)
    _, delta16, _ = awm.embed_waveform(x48, G, device=dev, messages=msgs, orig_freq=48000)
    assert tuple(delta16.shape) == (1, 32000 + 5000)
    check(delta, awm.resample(delta16, 16000, 48000)[:, :N], FWD_TOL, "delta at 48 kHz")
    # the waveform already on the device: the same result
    assert same((wm, delta, orig), awm.embed_waveform(x48.to(dev), G, device=dev, messages=msgs, orig_freq=48000, native_rate=True))
    # native_rate=False is the call without the keyword
    assert same(awm.embed_waveform(x48, G, device=dev, messages=msgs, orig_freq=48000, native_rate=False),
                awm.embed_waveform(x48, G, device=dev, messages=msgs, orig_freq=48000))
    # an empty recording
    wm0, d0, o0 = awm.embed_waveform(torch.zeros(2, 0), G, device=dev, orig_freq=48000, native_rate=True)
    assert tuple(wm0.shape) == (2, 0) and tuple(d0.shape) == (1, 0) and tuple(o0.shape) == (2, 0)
    # messages=None draws one message per segment
    wm_r, delta_r, _ = awm.embed_waveform(x48, G, device=dev, orig_freq=48000, native_rate=True)
    assert tuple(wm_r.shape) == (2, N) and bool(torch.isfinite(wm_r).all()) and torch.equal(wm_r, x48 + delta_r)


def test_generate_watermarked_audio_native_rate(awm, dev, models, tmp_path):
    G, _ = models
    N = int(44100 * 1.3)
    rng = np.random.default_rng(9)
    t = np.arange(N) / 44100.0
    pcm = np.stack([8000 * np.sin(2 * np.pi * 330 * t), 6000 * np.sin(2 * np.pi * 440 * t + 1)], axis=1) + rng.integers(-300, 300, size=(N, 2))
    pcm = pcm.astype("<i2")
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out" / "wm.wav")
    with wave.open(src, "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(44100); w.writeframes(pcm.tobytes())
    res = awm.generate_watermarked_audio(src, G, output_file=dst, device=dev, native_rate=True)
    assert set(res) == {"watermarked_waveform", "delta_waveform", "original_waveform", "metrics", "sample_rate"}
    assert res["sample_rate"] == 44100
    wm = res["watermarked_waveform"]
    assert tuple(wm.shape) == (2, N) and tuple(res["delta_waveform"].shape) == (1, N)
    assert np.array_equal(res["original_waveform"].numpy(), pcm.T.astype(np.float32) / 32768.0)
    back, rate = awm.read_audio(dst)
    assert rate == 44100 and tuple(back.shape) == (2, N)
    assert np.array_equal(back.numpy().view(np.uint32), wm.numpy().view(np.uint32)), "the file does not hold the returned samples bit for bit"
    assert set(res["metrics"]) == {"watermark_rms", "si_snr_db", "power_ratio_db"}
    assert all(math.isfinite(float(v)) for v in res["metrics"].values())
    assert res["metrics"]["watermark_rms"] == torch.sqrt((res["delta_waveform"] ** 2).mean()).item()
    assert res["metrics"]["si_snr_db"] == awm.compute_si_snr(res["original_waveform"], wm)
    # an in-memory waveform: the rate is orig_freq
    res_m = awm.generate_watermarked_audio(res["original_waveform"], G, device=dev, orig_freq=44100, native_rate=True)
    assert res_m["sample_rate"] == 44100 and tuple(res_m["watermarked_waveform"].shape) == (2, N)
    # without the keyword the dict has no new key
    res_old = awm.generate_watermarked_audio(src, G, device=dev)
    assert set(res_old) == {"watermarked_waveform", "delta_waveform", "original_waveform", "metrics"}
    assert tuple(res_old["watermarked_waveform"].shape) == (1, -((-16000 * N) // 44100))


def test_native_rate_at_16k_keeps_the_channels(awm, dev, models):
    G, _ = models
    N = 2 * 16000 + 5000
    x = signal("recording", 2, N, 16000, seed=91)
    msgs = torch.tensor([11, 22222, 65535])
    wm, delta, orig = awm.embed_waveform(x, G, device=dev, messages=msgs, native_rate=True)
    assert tuple(wm.shape) == (2, N) and tuple(delta.shape) == (1, N) and torch.equal(orig, x)
    assert torch.equal(wm, x + delta)
    # the model saw the mixdown: delta is what the 16 kHz call embeds into it
    mono = x.double().mean(dim=0, keepdim=True).float()
    _, delta_m, _ = awm.embed_waveform(mono, G, device=dev, messages=msgs)
    check(delta, delta_m, FWD_TOL, "delta of the mixdown")


# ------------------------------------------------------------------------------------------ B11. two streams at once
def test_two_streams(awm, dev):
    from awm_amd import ops
    Na, Nb = 48000 * 20 + 5, 44100 * 20 + 6
    xa = signal("noise", 2, Na, 48000, seed=95).to(dev)
    xb = signal("noise", 1, Nb, 44100, seed=96).to(dev)
    da = (0.01 * torch.randn(n_delta(Na, 48000), generator=torch.Generator().manual_seed(97))).to(dev)
    db = (0.01 * torch.randn(n_delta(Nb, 44100), generator=torch.Generator().manual_seed(98))).to(dev)
    ya, ua = ops.resample_add(xa, da, 48000)
    yb, ub = ops.resample_add(xb, db, 44100)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            a = ops.resample_add(xa, da, 48000)
        with torch.cuda.stream(s2):
            b = ops.resample_add(xb, db, 44100)
        outs.append((a, b))
    torch.cuda.synchronize()
    for (a, au), (b, bu) in outs:
        assert torch.equal(a, ya) and torch.equal(au, ua) and torch.equal(b, yb) and torch.equal(bu, ub)
