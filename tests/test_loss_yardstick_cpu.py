"""The input conditions of tests/loss_yardstick.py's case tables, asserted on the float64 references alone (no GPU): no reference value
lies within float32 round-off of a threshold, so tests/test_gpu_loss_stack.py cannot flake on a flipped mask bin, sign or clamp.  A
changed seed or torch version fails here.  Also: every reference is float64, and the tables the package hands the MEL and HF kernels
are what the oracle defines."""
import math

import numpy as np
import pytest
import torch

import loss_yardstick as Y
from oracle import wm_oracle as O


@pytest.mark.parametrize("B,T,seed", Y.LOUD_CASES)
def test_loud_inputs_keep_clear_of_the_mask_threshold(B, T, seed):
    clean, wm = Y.spectral_inputs("loud", B, T, seed)
    assert clean.shape == wm.shape == (B, 1, T) and T > 1024
    share, margin = Y.loud_margins(clean)
    print(f"loud ({B}, {T}) seed {seed}: share above the threshold {share:.3f}, margin {margin:.2e}")
    assert 0.2 <= share <= 0.8
    assert margin >= Y.LOUD_MARGIN
    # the float32 oracle's spectrum is round-off away: the margin is two orders of magnitude of room
    s32 = O._stft(clean.squeeze(1), 2048, 512).abs().double()
    s64 = O._stft(clean.double().squeeze(1), 2048, 512).abs()
    assert float((s32 - s64).abs().max()) * 50 <= Y.LOUD_MARGIN


@pytest.mark.parametrize("B,T,seed", Y.MEL_CASES)
def test_mel_inputs_keep_the_sign_of_the_log_mel_difference(B, T, seed):
    clean, wm = Y.spectral_inputs("mel", B, T, seed)
    assert clean.shape == wm.shape == (B, 1, T) and T > 512
    margin = Y.mel_margin(clean, wm)
    print(f"mel ({B}, {T}) seed {seed}: smallest |d| {margin:.2e}")
    assert margin >= Y.MEL_MARGIN


def test_hf_cases_cover_odd_and_even_frame_counts():
    frames = {T: 1 + T // 128 for _, T, _ in Y.HF_CASES}
    assert frames[257] == 3 and frames[384] == 4 and frames[1024] == 9 and frames[1100] == 9
    assert any(T % 128 == 0 for T in frames) and all(T > 256 for T in frames)


@pytest.mark.parametrize("kind,T,seed", Y.DEGENERATE_CASES)
def test_degenerate_batches_have_exactly_zero_gradient_rows_in_float64(kind, T, seed):
    clean, sig = Y.degenerate_inputs(kind, T, seed)
    if kind == "loud":
        share, margin = Y.loud_margins(clean[1:])
        assert 0.2 <= share <= 0.8 and margin >= Y.LOUD_MARGIN
    if kind == "mel":
        assert Y.mel_margin(clean[2:], sig[2:]) >= Y.MEL_MARGIN
    for dtype in (torch.float64, torch.float32):
        loss, grad = Y.spectral_ref(kind, clean, sig, dtype)
        assert loss.dtype == grad.dtype == dtype
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
        assert float(grad[:2].abs().max()) == 0.0
        assert float(grad[2].abs().max()) > 0.0


@pytest.mark.parametrize("kind,B,T,seed", Y.SPECTRAL_CASES)
def test_spectral_references_are_float64(kind, B, T, seed):
    clean, sig = Y.spectral_inputs(kind, B, T, seed)
    loss, grad = Y.spectral_ref(kind, clean, sig)
    assert loss.dtype == torch.float64 and grad.dtype == torch.float64 and grad.shape == (B, 1, T)
    assert float(loss) > 0.0 and bool(torch.isfinite(grad).all())
    l32, g32 = Y.spectral_ref(kind, clean, sig, torch.float32)
    assert l32.dtype == torch.float32 and g32.dtype == torch.float32
    # the float32 oracle is round-off away from it (no flipped threshold in the oracle either)
    assert Y.rel_err(l32, loss) <= 1e-5 and Y.rel_err(g32, grad) <= 1e-5


@pytest.mark.parametrize("kind", sorted(Y.STFT))
def test_torch_stft_refuses_half_a_window(kind):
    n_fft = Y.STFT[kind][0]
    x = torch.zeros(1, 1, n_fft // 2, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        Y.spectral_loss(kind, x, x)


# ------------------------------------------------------------------------------------------------------------ post-processing
def test_tap_sets():
    for name, n in (("package", 101), ("lowpass101", 101), ("random127", 127), ("single", 1)):
        k = Y.pp_taps(name)
        assert k.dtype == torch.float32 and k.shape == (n,)
        assert n == 1 or abs(float(k.double().sum()) - 1.0) <= 1e-6
    assert torch.equal(Y.pp_taps("package"), O.fir_kernel())
    k = Y.pp_taps("random127")
    assert float((k - k.flip(0)).abs().max()) > 0.05            # asymmetric: a flipped index shows
    # the low-pass is one: unit gain at DC, under 1e-2 at 6 kHz; the package's taps pass 6 kHz untouched
    w = np.exp(-2j * np.pi * 6000.0 / O.SAMPLE_RATE * np.arange(101))
    assert abs(np.dot(Y.pp_taps("lowpass101").double().numpy(), w)) <= 1e-2
    assert abs(abs(np.dot(Y.pp_taps("package").double().numpy(), w)) - 1.0) <= 1e-3


@pytest.mark.parametrize("tapset", Y.PP_TAPSETS)
@pytest.mark.parametrize("T", Y.PP_T)
def test_postproc_inputs_keep_clear_of_clamp_and_cap(T, tapset):
    taps = Y.pp_taps(tapset)
    for rows in Y.PP_ROWS:
        x = Y.pp_input(T, tapset, rows)
        assert x.shape == (Y.PP_B, 1, T)
        for stages in Y.PP_STAGES:
            cm, gm = Y.pp_margins(x, taps, stages, tapset)
            assert cm >= Y.CLAMP_MARGIN and gm >= Y.GAIN_MARGIN, (rows, stages, cm, gm)
            out, f, stats, grad = Y.pp_ref(x, taps, stages, Y.pp_upstream(T), tapset)
            assert out.dtype == f.dtype == stats.dtype == grad.dtype == torch.float64
        # which branches the rows take with all stages on: clamp and cap both bite at 0.03, neither at 0.001, and the all-zero
        # row's gain is exactly 1
        _, f, stats, _ = Y.pp_ref(x, taps, 7, None, tapset)
        for b, scale in enumerate(Y.PP_ROWS[rows]):
            if scale == 0.0:
                assert float(stats[b, 1]) == 1.0 and float(stats[b, 0]) == math.sqrt(Y.EPS)
            elif scale == 0.001:
                assert float(stats[b, 1]) == 1.0 and float(f[b].abs().max()) < Y.THR
            elif T >= 37:
                assert float(stats[b, 1]) < 1.0 and float(f[b].abs().max()) > Y.THR


@pytest.mark.parametrize("tapset", Y.PP_TAPSETS)
def test_postproc_input_at_the_length_limit(tapset):
    T = Y.PP_BIG_T
    x = Y.pp_input(T, tapset, "loud", 1)
    assert x.shape == (1, 1, T) and (T + 256) * 4 == 145024
    for stages in Y.PP_BIG_STAGES:
        cm, gm = Y.pp_margins(x, Y.pp_taps(tapset), stages, tapset)
        assert cm == math.inf and gm >= Y.GAIN_MARGIN


def test_package_taps_reference_is_the_oracle():
    x = Y.pp_input(100, "package", "loud")
    out, f, _, _ = Y.pp_ref(x, Y.pp_taps("package"), 7, None, "package")
    assert torch.equal(f, O.fir_lowpass(x.double()))
    assert torch.equal(out, O.limit_rms(O.clamp_peak(O.fir_lowpass(x.double()))))
    assert torch.equal(Y.pp_ref(x, Y.pp_taps("package"), 7, None, "package", torch.float32)[0], O.postprocess(x))


# ------------------------------------------------------------------------------------------------------------ BCE, L1, Adam
@pytest.mark.parametrize("NO", Y.BCE_NO)
def test_bce_reference(NO):
    for B, T in Y.BCE_BT:
        msg, x = Y.bce_messages(NO, B), Y.bce_logits(NO, B, T)
        assert msg.dtype == torch.int64 and msg.shape == (B,) and int(msg.min()) >= 0 and int(msg.max()) < 2 ** max(NO - 1, 1)
        assert x.shape == (2 * B, T, NO) and (T * NO) < 2 ** 23
        for r in (0, B):
            for o in (0, NO - 1):
                assert x[r, :5, o].tolist() == list(Y.PLANTED)
        for w in Y.BCE_WEIGHTS:
            loc, bce, grad = Y.bce_ref(x, msg, w)
            assert loc.dtype == grad.dtype == torch.float64 and (bce is None) == (NO == 1)
            assert bool(torch.isfinite(grad).all()) and math.isfinite(float(loc))
            l32, b32, g32 = Y.bce_ref(x, msg, w, torch.float32)
            assert Y.rel_err(l32, loc) <= 1e-6 and Y.rel_err(g32, grad) <= 1e-6
            if w[0] is None:
                assert float(grad[:, :, 0].abs().max()) == 0.0 and float(grad[B:].abs().max()) == 0.0
            if w[1] is None and NO > 1:
                assert float(grad[:, :, 1:].abs().max()) == 0.0
    if NO == 64:
        assert Y.bce_messages(64, 3).tolist() == [2 ** 63 - 1, 2 ** 62, 0]
        _, bits = Y.bce_targets(Y.bce_messages(64, 3), 64, 3, 1, torch.float64)
        assert bits[0].sum() == 63 and bits[1].sum() == 1 and bits[1, 0, 62] == 1 and bits[2].sum() == 0


def test_l1_inputs():
    for n in Y.L1_N:
        x = Y.l1_input(n)
        assert x.shape == (n,)
        if n >= 255:
            assert float(x[3]) == 0.0 and not math.copysign(1.0, float(x[3])) < 0 and math.copysign(1.0, float(x[n - 2])) < 0
    z = Y.l1_zero_input()
    assert math.copysign(1.0, float(z[0])) > 0 > math.copysign(1.0, float(z[1]))


@pytest.mark.parametrize("lr,betas,eps", Y.ADAM_HYPER)
def test_adam_reference_against_torch_in_float64(lr, betas, eps):
    """the float64 numpy step is torch.optim.Adam's step when that runs in float64"""
    n = 257
    for fresh, step0 in ((True, 1), (False, 1000)):
        p, m, v = Y.adam_state(n, 700, fresh)
        assert float(v.min()) >= 0.0 and (fresh or float(v.min()) > 0.0)
        for k in range(3):
            g = Y.adam_grad(n, 710 + k)
            assert float(g[5]) == 0.0 and abs(float(g[7]) - 1e-25) < 1e-32 and float(g[7]) ** 2 < 2.0 ** -149
            assert float(g.abs().max()) > 100.0 and 0.0 < float(g[g != 0].abs().min()) < 1e-12
            pr, mr, vr, upd = Y.adam_ref(p, g, m, v, lr, betas, eps, step0 + k)
            assert pr.dtype == mr.dtype == vr.dtype == upd.dtype == np.float64
            pt, mt, vt = Y.adam_torch_step(p.double(), g.double(), m.double(), v.double(), lr, betas, eps, step0 + k)
            assert pt.dtype == torch.float64
            room = p.double().abs() + m.double().abs() + v.double() + g.double().abs() + g.double() ** 2      # cancellation in m
            for a, r in ((pt, pr), (mt, mr), (vt, vr)):
                assert np.all(np.abs(a.numpy() - r) <= 1e-14 * (np.abs(r) + room.numpy()) + 1e-300)
            if fresh:
                assert pr[5] == float(p[5]) and mr[5] == 0.0 and vr[5] == 0.0
            p, m, v = (torch.from_numpy(a).float() for a in (pr, mr, vr))


# ------------------------------------------------------------------------------------------------------------ the package's tables
def test_mel_tables_are_the_oracles_filterbank_and_its_support():
    import awm_amd
    fb, klo, khi, mlo = awm_amd.losses._mel_tables("cpu")
    ref = O.mel_filterbank()
    assert fb.dtype == torch.float32 and fb.shape == (513, 64) and fb.is_contiguous()
    assert torch.equal(fb.view(torch.int32), ref.contiguous().view(torch.int32))
    nz = ref > 0
    for m in range(64):
        idx = torch.nonzero(nz[:, m]).flatten()
        assert idx.numel() > 0 and int(klo[m]) == int(idx[0]) and int(khi[m]) == int(idx[-1])
        assert bool(nz[int(idx[0]):int(idx[-1]) + 1, m].all())          # the support is one run: klo..khi is exactly it
    for k in range(513):
        idx = torch.nonzero(nz[k]).flatten()
        if idx.numel():
            assert int(mlo[k]) == int(idx[0]) and int(idx[-1]) - int(idx[0]) <= 2
        else:
            assert int(mlo[k]) == 0
    assert klo.dtype == khi.dtype == mlo.dtype == torch.int32


def test_hf_kcut_is_the_first_bin_above_the_cutoff(monkeypatch):
    import awm_amd
    seen = []
    monkeypatch.setattr(awm_amd.losses.ops._SpectralLossFn, "apply", staticmethod(lambda *a: seen.append(a)))
    awm_amd.losses.high_freq_penalty(torch.zeros(1, 1, 512))
    (kind, _, _, kcut), = seen
    freqs = torch.fft.rfftfreq(512, 1 / O.SAMPLE_RATE)
    first = int(torch.nonzero(freqs > 3500.0).flatten()[0])
    assert kind == "hf" and kcut == first == 113
    assert float(freqs[first - 1]) <= 3500.0 < float(freqs[first])
