"""The 16-bit save path and main15c's codec on the GPU: wm_biquad (csrc/biquad.hip) runs a biquad section along rows of any length as
time-parallel chunks (or one lane per row where the warm-up would be too long), with the clamp, the 16-bit rounding or the int16 cast as
its epilogue; `ops.biquad`, `ops.PcmCodecFn`, `perceptual_postprocess`, `PcmCodec`, `encode_pcm16`, `save_audio(device=)` and the
`codec=` keyword of the step functions on top of it.

The yardstick is `yardstick()` of tests/biquad_yardstick.py, float64 scipy.signal.lfilter with nothing from the package; the derived
tolerance of the float mode stands in that module's docstring.

The int16 codes are compared with trunc(clamp(y64) * 32767): a truncating cast after a recursive filter cannot be bit-identical between two
evaluation orders, so every difference must be +-1 and at most 1 % of the samples may differ (a condition, not a measurement).  Given
the kernel's own float output the two quantisers are exact, and are held to bit identity."""
import copy
import math
import wave

import numpy as np
import pytest
import torch

from biquad_yardstick import yardstick
from gpu_support import awm, dev  # noqa: F401
from gpu_support import reference_models, rel_err
from oracle import wm_oracle as O
from yardstick_common import assert_within

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4
PAIRS = [(16000, 7000), (44100, 7000), (48000, 7000), (48000, 500), (16000, 50)]
LENGTHS = [1, 2, 3, 63, 64, 65, 1000, 4097, 40000]
KINDS = ["noise", "tonal", "impulse", "loud"]
ROWS = 3


# ------------------------------------------------------------------------------------------ inputs and their shared references
def signal(kind, n, rate, seed=0):
    """(ROWS, n) float32 CPU"""
    g = torch.Generator().manual_seed(1000 * seed + n)
    if kind == "noise":
        return 0.3 * torch.randn(ROWS, n, generator=g)
    if kind == "loud":                                                                        # the clamp acts
        return 3.0 * torch.randn(ROWS, n, generator=g)
    if kind == "tonal":
        t = torch.arange(n, dtype=torch.float64) / rate
        x = 0.8 * sum(a * torch.sin(2 * math.pi * f * t + p) for a, f, p in ((0.4, 220.0, 0.1), (0.2, 1730.0, 1.0), (0.1, 5200.0, 2.0)))
        return (x[None, :].repeat(ROWS, 1) * torch.linspace(1.0, 0.6, ROWS, dtype=torch.float64)[:, None]).float() + \
            0.01 * torch.randn(ROWS, n, generator=g)
    x = torch.zeros(ROWS, n)                                                                  # impulse: first sample | last sample | both
    x[0, 0] = 1.0
    x[1, n - 1] = 1.0
    x[2, 0] = 0.75
    x[2, n - 1] += 0.5
    return x


_REF = {}


def reference(rate, cutoff, kind, n, W):
    """(x (ROWS, n) CPU float32, y64, bound): computed once per case, shared by every test that needs it, never written to"""
    key = (rate, cutoff, kind, n)
    if key not in _REF:
        x = signal(kind, n, rate)
        y64, bound = yardstick(x.numpy(), rate, cutoff, W)
        _REF[key] = (x, y64, bound)
    return _REF[key]


def bits_of(mask, n):
    """int32 words (rows, ceil(n / 32)) -> bool (rows, n)"""
    m = mask.cpu().numpy().astype(np.uint32)
    return torch.from_numpy(((m[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(m.shape[0], -1)[:, :n].astype(bool))


# ------------------------------------------------------------------------------------------ 1. float mode against the yardstick
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rate,cutoff", PAIRS)
def test_float_mode_vs_yardstick(awm, dev, rate, cutoff, kind):
    from awm_amd import ops
    coeffs = ops.biquad_lowpass_coeffs(rate, cutoff)
    W = ops.biquad_warm(coeffs)
    warm, chunk = ops.biquad_plan(coeffs)
    if (rate, cutoff) == (16000, 50):
        assert (warm, chunk) == (-1, 0), "16 kHz / 50 Hz must take the one-lane-per-row form"
    else:
        assert warm == W and chunk > 0, "the 7 kHz and 500 Hz sections must take the chunked form"
    for n in LENGTHS:
        x, y64, bound = reference(rate, cutoff, kind, n, W)
        xd = x.to(dev)
        for rows in (1, 2, 3):
            y = ops.biquad(xd[:rows], coeffs, clamp=False)
            assert y.shape == (rows, n) and y.dtype == torch.float32
            assert_within(y.cpu().numpy(), y64[:rows], bound[:rows], f"{rate}/{cutoff} {kind} rows={rows} n={n} clamp off")
            yc = ops.biquad(xd[:rows], coeffs, clamp=True)
            assert_within(yc.cpu().numpy(), np.clip(y64[:rows], -1.0, 1.0), bound[:rows], f"{rate}/{cutoff} {kind} rows={rows} n={n} clamp on")
            assert torch.equal(yc, y.clamp(-1.0, 1.0)), "the clamp is an epilogue of the same recursion"
    if kind == "loud" and cutoff == 7000:
        assert float(np.abs(y64).max()) > 1.0, "this input is meant to drive the clamp"


# ------------------------------------------------------------------------------------------ 2. chunk seams
@pytest.mark.parametrize("rate,cutoff", PAIRS[:4])
def test_chunk_seams(awm, dev, rate, cutoff):
    """an impulse just before, on and just after the first seam, and at the start of a warm-up: the smallest case in which a lost or
    doubled warm-up shows.  Lc - W is the start of the warm-up of the chunk behind the first seam; where the op's chunks are shorter than
    the warm-up (Lc < W) that position lies before the row, so the first seam whose warm-up starts inside the row, k Lc - W with
    k = ceil(W / Lc), stands in for it (k = 1 where Lc >= W), together with the samples on either side of it."""
    from awm_amd import ops
    coeffs = ops.biquad_lowpass_coeffs(rate, cutoff)
    W, Lc = ops.biquad_plan(coeffs)
    assert W == ops.biquad_warm(coeffs) and Lc > 0
    k = max(1, -(-W // Lc))
    spots = sorted({Lc - 1, Lc, Lc + 1, k * Lc - W, max(0, k * Lc - W - 1), k * Lc - W + 1})
    n = (k + 4) * Lc + 7
    x = torch.zeros(len(spots), n)
    for r, p in enumerate(spots):
        x[r, p] = 0.9
    y64, bound = yardstick(x.numpy(), rate, cutoff, W)
    y = ops.biquad(x.to(dev), coeffs, clamp=False)
    assert_within(y.cpu().numpy(), y64, bound, f"{rate}/{cutoff} seams Lc={Lc} W={W} impulses at {spots}")


# ------------------------------------------------------------------------------------------ 3. shape and layout
def test_batch_shape_equals_rows(awm, dev):
    from awm_amd import ops
    coeffs = ops.biquad_lowpass_coeffs(16000, 7000)
    x = (0.3 * torch.randn(4, 16000, generator=torch.Generator().manual_seed(5))).to(dev)
    for mode in ("float", "round", "pcm16"):
        a = ops.biquad(x.view(4, 1, 16000), coeffs, mode=mode)
        b = ops.biquad(x, coeffs, mode=mode)
        assert a.shape == (4, 1, 16000) and torch.equal(a.view(4, 16000), b), mode
        assert torch.equal(ops.biquad(x, coeffs, mode=mode), b), f"{mode}: two runs differ"
    v = ops.biquad(x[0], coeffs)
    assert v.shape == (16000,) and torch.equal(v, ops.biquad(x[:1], coeffs)[0])


@pytest.mark.parametrize("rate,cutoff", [(16000, 7000), (16000, 50)])
@pytest.mark.parametrize("reverse", [False, True])
def test_unaligned_buffers_and_guards(awm, dev, rate, cutoff, reverse):
    """buffers that start 1 and 3 floats (int16: 1 and 3 codes) into their allocations give the bits of aligned ones, and nothing outside
    `out` or the mask is written (the launcher is called with hand-made buffers so that the mask has guard words too)"""
    from awm_amd import ops
    coeffs = ops.biquad_lowpass_coeffs(rate, cutoff)
    warm, _ = ops.biquad_plan(coeffs)
    G = 64
    for rows, n in ((3, 4097), (2, 1000), (1, 33)):
        x = 1.5 * torch.randn(rows, n, generator=torch.Generator().manual_seed(n))
        nw = (n + 31) // 32
        for mode, odt, sentinel in (("float", torch.float32, 777.0), ("round", torch.float32, 777.0), ("pcm16", torch.int16, 12345)):
            want_mask = not reverse
            res = ops.biquad(x.to(dev), coeffs, mode=mode, reverse=reverse, mask_out=want_mask)
            ref, ref_mask = res if want_mask else (res, None)
            for off in (1, 3):
                xb = torch.full((rows * n + 8,), float("nan"), device=dev)
                xv = xb[off:off + rows * n].view(rows, n)
                xv.copy_(x)
                ob = torch.full((rows * n + 2 * G,), sentinel, dtype=odt, device=dev)
                mb = torch.full((rows * nw + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
                ov = ob[G + off:G + off + rows * n]
                mv = mb[G + off:G + off + rows * nw]
                awm.lib.wm_biquad(xv.data_ptr(), ov.data_ptr(), mv.data_ptr() if want_mask else None, None, *coeffs, rows, n, warm,
                                  ops.BIQUAD_MODES[mode], 1, int(reverse), torch.cuda.current_stream().cuda_stream)
                what = f"{rate}/{cutoff} {mode} reverse={reverse} rows={rows} n={n} offset {off}"
                assert torch.equal(ov.view(rows, n), ref), what
                assert bool((ob[:G + off] == sentinel).all()) and bool((ob[G + off + rows * n:] == sentinel).all()), f"{what}: guard of out"
                if want_mask:
                    assert torch.equal(mv.view(rows, nw), ref_mask), f"{what}: mask"
                    assert bool((mb[:G + off] == 0x5A5A5A5A).all()) and bool((mb[G + off + rows * nw:] == 0x5A5A5A5A).all()), f"{what}: guard of mask"
                else:
                    assert bool((mb == 0x5A5A5A5A).all())
                # the `out=` keyword of the op writes the same bits into a caller's buffer
                o2 = torch.empty(rows, n, dtype=odt, device=dev)
                assert ops.biquad(xv, coeffs, mode=mode, reverse=reverse, out=o2) is o2 and torch.equal(o2, ref), what


# ------------------------------------------------------------------------------------------ 4. reverse
@pytest.mark.parametrize("rate,cutoff", [(16000, 7000), (48000, 500), (16000, 50)])
def test_reverse_is_flip_filter_flip(awm, dev, rate, cutoff):
    from awm_amd import ops
    coeffs = ops.biquad_lowpass_coeffs(rate, cutoff)
    for n in (1, 2, 31, 65, 1000, 4097, 40000):
        x = signal("loud", n, rate, seed=3).to(dev)
        for mode in ("float", "round", "pcm16"):
            r = ops.biquad(x, coeffs, mode=mode, reverse=True)
            f = ops.biquad(x.flip(-1).contiguous(), coeffs, mode=mode).flip(-1)
            assert torch.equal(r, f), f"{rate}/{cutoff} n={n} {mode}"


# ------------------------------------------------------------------------------------------ 5. the quantisers, given the filter output
def tie_samples():
    """float32 values v with float32(v * 32767) exactly k + 0.5 (searched, not assumed), both signs, plus +-1, values beyond the clamp and zeros"""
    out = []
    for k in list(range(0, 64)) + [100, 1000, 16383, 16384, 20000, 32765, 32766]:
        v = np.float32((k + 0.5) / 32767.0)
        for cand in (v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(2))):
            if np.float32(cand * np.float32(32767.0)) == np.float32(k + 0.5):
                out += [float(cand), -float(cand)]
                break
    assert len(out) >= 40, "the search found too few exact ties"
    return out + [1.0, -1.0, 1.5, -1.5, 0.0, -0.0, 0.99999994, -0.99999994, 1.0 / 32767, 3.0517578125e-05]


def test_quantisers_exact_given_filter_output(awm, dev):
    from awm_amd import ops
    ties = torch.tensor(tie_samples(), dtype=torch.float32)
    ties = torch.cat([ties, 0.7 * torch.randn(4097 - ties.numel() % 4097, generator=torch.Generator().manual_seed(9))]).view(1, -1)
    cases = [(ops.BIQUAD_IDENTITY, ties)]                                         # the quantiser alone: y = x, ties land where they were put
    for rate, cutoff in ((16000, 7000), (48000, 7000), (16000, 50)):
        cases.append((ops.biquad_lowpass_coeffs(rate, cutoff), signal("loud", 40000, rate, seed=4)))
        cases.append((ops.biquad_lowpass_coeffs(rate, cutoff), signal("tonal", 4097, rate, seed=4)))
    for coeffs, x in cases:
        xd = x.to(dev)
        yf = ops.biquad(xd, coeffs).cpu()
        if coeffs == ops.BIQUAD_IDENTITY:
            assert torch.equal(yf, x.clamp(-1.0, 1.0))
        rd = ops.biquad(xd, coeffs, mode="round").cpu()
        pc = ops.biquad(xd, coeffs, mode="pcm16").cpu()
        assert pc.dtype == torch.int16
        assert torch.equal(rd, torch.round(yf * 32767) / 32767), "mode round"
        assert torch.equal(pc, (yf * 32767).to(torch.int16)), "mode pcm16"


# ------------------------------------------------------------------------------------------ 6. codes against the float64 yardstick
@pytest.mark.parametrize("kind", ["noise", "tonal"])
@pytest.mark.parametrize("rate", [16000, 44100, 48000])
def test_codes_vs_float64(awm, dev, rate, kind):
    from awm_amd import ops
    coeffs = ops.biquad_lowpass_coeffs(rate, 7000)
    x, y64, _ = reference(rate, 7000, kind, 40000, ops.biquad_warm(coeffs))
    want = np.trunc(np.clip(y64, -1.0, 1.0) * 32767.0).astype(np.int64)
    got = awm.encode_pcm16(x.to(dev), rate, 7000)
    assert got.dtype == torch.int16 and got.is_cuda and got.shape == x.shape
    assert torch.equal(got, ops.biquad(x.to(dev), coeffs, mode="pcm16"))
    diff = got.cpu().numpy().astype(np.int64) - want
    share = float((diff != 0).mean())
    print(f"{rate} Hz {kind}: codes differ in {100 * share:.3f} % of samples, max |diff| {np.abs(diff).max()}")
    assert np.abs(diff).max() <= 1, "a code is more than one step from the float64 code"
    assert share <= 0.01, f"{100 * share:.3f} % of the codes differ from float64"


def test_save_audio_on_device(awm, dev, tmp_path):
    """save_audio(device="cuda") writes encode_pcm16's codes, interleaved; device=None keeps the host path also for a CUDA waveform"""
    x = signal("tonal", 40000, 48000, seed=6)[:2]
    a, b, c = (str(tmp_path / f"{k}.wav") for k in "abc")
    awm.save_audio(x, a, 48000, device="cuda")
    awm.save_audio(x.to(dev), b, 48000, device="cuda")
    awm.save_audio(x.to(dev), c, 48000)
    codes = awm.encode_pcm16(x.to(dev), 48000).cpu().numpy()
    host = awm.pcm16(awm.lowpass_biquad(x, 48000, 7000)).numpy()
    for path, want in ((a, codes), (b, codes), (c, host)):
        with wave.open(path, "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (2, 2, 48000, 40000)
            got = np.frombuffer(w.readframes(40000), dtype="<i2").reshape(-1, 2).T
        assert np.array_equal(got, want), path
    assert np.abs(codes.astype(np.int64) - host.astype(np.int64)).max() <= 1
    q = awm.encode_pcm16(x.to(dev), 48000, lowpass_hz=None)
    assert torch.equal(q.cpu(), awm.pcm16(x))


# ------------------------------------------------------------------------------------------ 7. masks
@pytest.mark.parametrize("rate,cutoff", [(16000, 7000), (16000, 50)])
def test_masks(awm, dev, rate, cutoff):
    from awm_amd import ops
    coeffs = ops.biquad_lowpass_coeffs(rate, cutoff)
    for n in (1, 31, 32, 33, 1000, 4097, 40000):
        x = signal("loud", n, rate, seed=7).to(dev)
        if cutoff == 50:
            x = x * 40.0                                                             # a 50 Hz section passes little of white noise
        raw = ops.biquad(x, coeffs, clamp=False)
        for mode in ("float", "round", "pcm16"):
            out, mask = ops.biquad(x, coeffs, mode=mode, mask_out=True)
            assert mask.dtype == torch.int32 and mask.shape == (ROWS, (n + 31) // 32)
            assert torch.equal(out, ops.biquad(x, coeffs, mode=mode))
            keep = bits_of(mask, n)
            assert torch.equal(keep, (raw.abs() <= 1.0).cpu()), f"{rate}/{cutoff} n={n} {mode}"
            pad_bits = bits_of(mask, 32 * mask.shape[1])[:, n:]
            assert not bool(pad_bits.any()), "bits behind the row are zero"
        if n >= 1000:
            assert 0 < int(keep.sum()) < keep.numel(), "the clamp must act on some samples and spare others"
        for reverse in (False, True):
            a = ops.biquad(x, coeffs, clamp=False, reverse=reverse, mask_in=mask)
            b = ops.biquad(x * keep.to(dev).float(), coeffs, clamp=False, reverse=reverse)
            assert torch.equal(a, b), f"mask_in {rate}/{cutoff} n={n} reverse={reverse}"


# ------------------------------------------------------------------------------------------ 8. gradients
@pytest.mark.parametrize("rate,cutoff", [(16000, 7000), (16000, 50)])
def test_straight_through_backward(awm, dev, rate, cutoff):
    """gx = flip(lfilter64(flip(g * mask))): rounding passes g, the clamp where |y| <= 1, the filter through its adjoint.  The bound is the
    yardstick's, evaluated on the flipped data."""
    from awm_amd import ops
    coeffs = ops.biquad_lowpass_coeffs(rate, cutoff)
    W = ops.biquad_warm(coeffs)
    n = 4097
    x = signal("loud", n, rate, seed=8) * (40.0 if cutoff == 50 else 1.0)
    g = signal("noise", n, rate, seed=9)
    xd = x.view(ROWS, 1, n).to(dev).requires_grad_()
    out = awm.perceptual_postprocess(xd, cutoff, rate, grad="straight_through")
    assert out.requires_grad and torch.equal(out.detach(), ops.biquad(xd.detach(), coeffs, mode="round"))
    out.backward(g.view(ROWS, 1, n).to(dev))
    keep = (ops.biquad(xd.detach(), coeffs, clamp=False).abs() <= 1.0).view(ROWS, n).cpu()
    assert 0 < int(keep.sum()) < keep.numel()
    gm = (g * keep.float()).numpy()
    y64, bound = yardstick(gm[:, ::-1], rate, cutoff, W)
    assert_within(xd.grad.view(ROWS, n).cpu().numpy(), y64[:, ::-1], bound[:, ::-1], f"{rate}/{cutoff} straight-through gx")
    # the module form, and the reference mode: no gradient at all
    codec = awm.PcmCodec(cutoff, rate, grad="straight_through")
    assert torch.equal(codec(xd).detach(), out.detach())
    ref = awm.PcmCodec(cutoff, rate)(xd)
    assert not ref.requires_grad and torch.equal(ref, out.detach())


def test_train_step_reference_gradient_mode(awm, dev, monkeypatch):
    """main15c's step: s_w = codec(s + delta) feeds the Detector, mel and loudness; with torch.round's zero gradient only l1 and hf train
    the Generator, the Detector trains on the processed signal, and nothing leaves the device on the way"""
    from awm_amd import step
    G, D = reference_models(awm, dev)
    G2, D2 = copy.deepcopy(G), copy.deepcopy(D)
    for m in (G, D, G2, D2):
        m.train()
    B, T = 2, 2048
    s = O.synthetic_clips(B, seed=31, T=T).to(dev)
    msg = torch.tensor([3, 60001], device=dev)
    opt = torch.optim.Adam(list(G.parameters()) + list(D.parameters()), lr=1e-3)
    codec = awm.PcmCodec()

    def no_download(mp, name):
        orig = getattr(torch.Tensor, name)

        def guarded(self, *a, **k):
            assert not self.is_cuda, f"Tensor.{name}() on a device tensor inside the step"
            return orig(self, *a, **k)
        mp.setattr(torch.Tensor, name, guarded)
    with monkeypatch.context() as mp:
        for name in ("cpu", "item", "numpy", "tolist"):
            no_download(mp, name)
        out = awm.train_step(G, D, opt, s, msg, codec=codec)
    assert all(v.is_cuda for v in out.values())
    assert not out["s_w"].requires_grad
    assert torch.equal(out["s_w"], awm.perceptual_postprocess(s + out["delta"].detach()))
    assert not torch.equal(out["s_w"], s + out["delta"].detach())
    # the Generator: gradients of w_l1 l1 + w_hf hf alone, from a run without the codec on a copy
    _, out2 = step.forward_losses(G2, D2, s, msg)
    (step.LOSS_WEIGHTS["l1"] * out2["l1"] + step.LOSS_WEIGHTS["hf"] * out2["hf"]).backward()
    p2 = dict(G2.named_parameters())
    for k, p in G.named_parameters():
        assert p.grad is not None and p2[k].grad is not None, k
        e = rel_err(p.grad, p2[k].grad)
        assert e <= FWD_TOL, f"Generator {k}: gradient differs from the l1 + hf gradient by {e:.3e}"
    for k, p in D.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), f"Detector {k}"


def _same(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_codec_none_is_todays_graph(awm, dev):
    from awm_amd import step
    G, D = reference_models(awm, dev)
    s = O.synthetic_clips(2, seed=33, T=2048).to(dev)
    msg = torch.tensor([7, 4242], device=dev)
    G.train(); D.train()
    _same(step.forward_losses(G, D, s, msg)[1], step.forward_losses(G, D, s, msg, codec=None)[1])
    G.eval(); D.eval()
    _same(awm.eval_forward(G, D, s, msg), awm.eval_forward(G, D, s, msg, codec=None))
    assert "s_w" not in awm.eval_forward(G, D, s, msg)


def test_eval_forward_codec_on_both_branches(awm, dev):
    G, D = reference_models(awm, dev)
    G.eval(); D.eval()
    s = O.synthetic_clips(2, seed=35, T=2048).to(dev)
    msg = torch.tensor([9, 777], device=dev)
    codec = awm.PcmCodec()
    a = awm.eval_forward(G, D, s, msg, codec=codec)                               # overlapped: the clean half runs beside the Generator
    assert torch.equal(a["s_w"], awm.perceptual_postprocess(s + a["delta"]))
    with torch.no_grad():
        assert torch.equal(a["logits"][:2], D(a["s_w"])), "the Detector must see the processed signal"
    assert not torch.equal(a["logits"], awm.eval_forward(G, D, s, msg)["logits"])
    D.training = True                                                             # the flag of the top module alone: every layer stays in eval mode,
    try:                                                                          # but eval_forward takes its plain (single 2B-row call) branch
        b = awm.eval_forward(G, D, s, msg, codec=codec)
    finally:
        D.training = False
    _same(a, b)
    ev = awm.evaluate_batches(G, D, [s.cpu()], device=dev, messages=[msg.cpu()], codec=codec)
    assert abs(ev["watermarked_prob"] - float(a["prob_watermarked"].double().mean())) < 1e-6


# ------------------------------------------------------------------------------------------ 9. argument errors
def test_argument_errors_launch_nothing(awm, dev, monkeypatch):
    from awm_amd import ops
    coeffs = ops.biquad_lowpass_coeffs(16000, 7000)
    awm.lib.load()
    real = awm.lib.wm_biquad
    launches = []
    monkeypatch.setattr(awm.lib, "wm_biquad", lambda *a: launches.append(a), raising=False)
    base = torch.zeros(3000, device=dev)
    x = base[:2000].view(2, 1000)
    with pytest.raises(ValueError):
        ops.biquad(x, coeffs, out=base[1000:3000].view(2, 1000))
    with pytest.raises(ValueError):
        ops.biquad(x, coeffs, out=x)
    with pytest.raises(ValueError):
        ops.biquad(torch.zeros(0, 10, device=dev), coeffs)
    with pytest.raises(ValueError):
        ops.biquad(torch.zeros(3, 0, device=dev), coeffs)
    with pytest.raises(ValueError):
        ops.biquad(torch.zeros(2, 100), coeffs)
    with pytest.raises(ValueError):
        ops.biquad(x, coeffs, mode="pcm24")
    with pytest.raises(ValueError):
        ops.biquad(x, coeffs, mask_out=True, reverse=True)
    for bad in ((0, 7000), (-16000, 7000), (16000, 0), (16000, 8000), (16000, 9000), (float("nan"), 7000), ("16k", 7000)):
        with pytest.raises(ValueError):
            ops.biquad_lowpass_coeffs(*bad)
        with pytest.raises(ValueError):
            awm.perceptual_postprocess(x, bad[1], bad[0])
        with pytest.raises(ValueError):
            awm.PcmCodec(bad[1], bad[0])
    with pytest.raises(ValueError):
        awm.perceptual_postprocess(x, grad="ste")
    assert launches == [], "a rejected call reached the launcher"
    monkeypatch.setattr(awm.lib, "wm_biquad", real, raising=False)
    # the launcher's own checks: hipErrorInvalidValue (1) before any launch
    o = torch.full((2, 1000), 5.0, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    for args in ((x.data_ptr(), o.data_ptr(), None, None, *coeffs, 0, 1000, 100, 0, 1, 0, st),
                 (x.data_ptr(), o.data_ptr(), None, None, *coeffs, 2, 0, 100, 0, 1, 0, st),
                 (None, o.data_ptr(), None, None, *coeffs, 2, 1000, 100, 0, 1, 0, st),
                 (x.data_ptr(), None, None, None, *coeffs, 2, 1000, 100, 0, 1, 0, st),
                 (x.data_ptr(), x.data_ptr() + 4000, None, None, *coeffs, 2, 1000, 100, 0, 1, 0, st),
                 (x.data_ptr(), o.data_ptr(), None, None, *coeffs, 2, 1000, 100, 2, 0, 0, st),
                 (x.data_ptr(), o.data_ptr(), None, None, *coeffs, 2, 1000, 5000, 0, 1, 0, st)):
        with pytest.raises(RuntimeError, match="hipError 1"):
            awm.lib.wm_biquad(*args)
    torch.cuda.synchronize()
    assert bool((o == 5.0).all())
