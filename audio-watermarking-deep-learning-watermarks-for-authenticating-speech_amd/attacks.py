"""Channel distortions between s + delta and the Detector, and the loop that tells how detection moves under them.

The reference README's "Robustness Testing" section promises a watermark that survives compression, resampling, volume changes and
additive noise; it ships no code for the last two, and no codec to train against.  Here they are modules on (B, 1, T), (C, N) or (N,)
that go wherever codec.PcmCodec goes -- the `codec=` argument of forward_losses / train_step / eval_forward / evaluate_batches takes any of them, and chains are plain
torch.nn.Sequential(Distortion(...), PcmCodec(...)), which therefore already works as `codec=`:

  Distortion   per-clip gain and white Gaussian noise at a set SNR: one wm_distort call (dsp.DistortFn), differentiable
  Lowpass      the biquad low-pass alone (no clamp, no 16-bit grid): dsp.biquad, its backward the same launch with reverse=True
  Resampled    down to another rate and back (8 kHz telephony, say), every row by itself: two wm_resample_rows launches
               (dsp.ResampleRowsFn), the backward of each the same launch with the transposed table
  TransformCodec   a STAND-IN for lossy compression: lapped MDCT, per-band quantiser at a per-row SNR, bandwidth cut, synthesis -- one
               wm_mdct_codec launch (dsp.MdctCodecFn), its backward the same launch with the quantiser off.  The signal path MP3 / AAC
               share, not an encoder: parity with a real one is unmeasured
  LpcCodec     a STAND-IN for a predictive speech codec (ADPCM / CELP / AMR-WB / SILK are all linear-predictive): per-frame LPC, an
               open-loop quantiser on the prediction residual at a per-row SNR, all-pole synthesis that shapes the noise like the
               speech envelope -- one wm_lpc_codec launch (dsp.LpcCodecFn); its "dead_zone" backward is the adjoint launch.  No LSP
               interpolation, no pitch predictor, no noise feedback, no entropy coder: parity with a real codec is unmeasured
  NoiseSuppress   the REMOVAL attack, a STAND-IN for a single-channel noise suppressor: a short-time spectral Wiener gate with a
               decision-directed a-priori SNR against one stationary noise estimate per row, at most reduce_db dB of attenuation per bin
               drawn per row -- one wm_noise_suppress call (suppress.NoiseSuppressFn); with the gains held the map is self-adjoint, so
               its backward is the same call on dy.  No voice-activity detector, no minimum statistics, no neural denoiser: parity with
               WebRTC NS, RNNoise, `noisereduce` or any product's suppressor is unmeasured
  Convolved    a long convolutive channel: every row convolved with a given impulse response, or with one drawn per row from a bank of
               measured ones -- one wm_fir_rows launch (dsp.FirRowsFn), its backward the same launch with reverse=True.  echo_ir
               makes the two-tap response of a plain echo
  Reverb       the same launch with SYNTHETIC room responses drawn on the device per row (wm_rir_synth) at a per-row RT60 and
               direct-to-reverberant ratio: exponentially decaying Gaussian noise, not a room simulation -- survival in real rooms
               is unmeasured
  TimeWarp     the desynchronising channel: playback at another speed (tempo and pitch together), sinusoidal wow / flutter and a cut at
               the front, through a Hann-windowed sinc interpolator whose phase is computed per output sample -- one wm_time_warp launch
               (dsp.TimeWarpFn), its backward the same launch with adjoint=True.  Survival against real players and tapes is
               unmeasured
  TimeStretch  the pitch-preserving change of tempo: waveform-similarity overlap-add (WSOLA), frames copied from near their nominal
               place to evenly spaced places of the output and cross-faded -- one wm_wsola launch (dsp.WsolaFn), its backward the
               same launch as a gather with the chosen positions held constant.  A piecewise copy with cross-faded jumps, a
               rectangular search, no transient detection: parity with any real editor's stretch is unmeasured
  PitchShift   the change of pitch at constant tempo: TimeStretch by 1 / beta followed by wm_time_warp at speed beta, no kernel of
               its own
  evaluate_robustness   watermarked / clean probability, bit accuracy and delta RMS per attack, pooled as evaluate_batches pools them
  Splice       the EDITING attack, and the only module here with two inputs: spans of the watermarked signal are cut out and replaced by
               the clean signal, by silence, or by clean audio moved from elsewhere in the same row -- one wm_splice launch
               (dsp.SpliceFn) that also emits the per-sample labels "still watermarked" as a bit mask; its backward passes the
               gradient where the label is 1.  It is the `tamper=` argument of forward_losses / train_step / eval_forward /
               evaluate_batches, NOT a `codec=` and not a member of Sequential chains.  Rectangular cuts without a crossfade, "moved"
               audio from the same row only; whether a model trained with it localises real edits is unmeasured
  evaluate_localization   IoU, precision, recall and sample accuracy of the per-sample track against Splice's labels, from integer counts

The modules are here, with their argument checks and the evaluation loops.  The random numbers they draw are counter-based, so nothing is
stored for the backward pass and a run is reproducible from `seed`; draws.py restates on the host exactly the numbers the kernels draw
and holds the table of which attack owns which output word (draws.WORDS: a new attack takes a free cell of it).  What a CPU tensor runs
in place of a kernel is in attacks_host.py.  Both modules' names are bound here too: attacks.<name> is their public spelling."""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch

from . import dsp, suppress
from ._host import _chk_int, _chk_positive
from .attacks_host import (  # noqa: F401  what a CPU tensor runs lives in attacks_host.py; attacks.<name> stays its spelling
    _conv_rows_host, _gather_ext, _lpc_rows_host, _sinpi, _warp_rows_host, _wsola_rows_host, distort_rows_host, mdct_codec_rows_host,
    pack_labels, splice_rows_host, unpack_labels)
from .codec import SAMPLE_RATE, _time_rows
from .draws import (  # noqa: F401  the host-side draws live in draws.py; attacks.<name> stays their public spelling
    _M0, _M1, _W0, _W1, FAMILIES, SPLICE_KINDS, WORDS, _affine, _check_cut, _key, _normals, _unit, _words, normal_noise, philox4x32_10,
    rir_taps, row_bank_index, row_lpc_snr_db, row_parameters, row_pitch_params, row_reduce_db, row_reverb_params, row_snr_db,
    row_splice_spans, row_stretch_rates, row_warp_params)
from .losses import postprocess

NOISE_GRAD_MODES = ("through", "detached")


def _pair(v, name):
    pair = tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if len(pair) != 2 or not all(isinstance(b, (int, float)) and not isinstance(b, bool) and math.isfinite(b) for b in pair):
        raise ValueError(f"{name}: expected a finite number or a (low, high) pair of them, got {v!r}")
    lo, hi = pair
    if lo > hi:
        raise ValueError(f"{name}: low {lo} is above high {hi}")
    return float(lo), float(hi)


class _RowDraws(torch.nn.Module):
    """What the per-row random modules share: `seed`, the running `draw` with reset(draw), the numbering of rows from `row0`, and the
    step to the next draw.  A forward checks its arguments first and steps last, so a call that raises consumes no draw."""

    def __init__(self, seed):
        super().__init__()
        self.seed = _chk_int(seed, "seed", what="an int")
        self.reset()

    def reset(self, draw=0):
        self.draw = _chk_int(draw, "draw", 0, 2 ** 32 - 1, "an int in [0, 2^32)")
        return self

    def _rows(self, x, row0):
        """x as time rows, their number, and the row numbers row0 + r the draws take; row0 + rows must stay a row counter"""
        x = _time_rows(x, "x")
        rows = x.numel() // x.shape[-1]
        _chk_int(row0, "row0", 0, 2 ** 32 - rows, "an int with 0 <= row0 and row0 + rows <= 2^32")
        return x, rows, row0 + np.arange(rows)

    def _next_draw(self):
        draw, self.draw = self.draw, (self.draw + 1) % 2 ** 32
        return draw


class Distortion(_RowDraws):
    """y = g x + s z for every row (clip or channel) of x, (B, 1, T), (C, N) or (N,):  g = 10^(gain_db / 20) with gain_db drawn uniformly
    from the pair `gain_db` per row, z white Gaussian noise at an SNR of snr_db (drawn from the pair `snr_db`) against g x, added to a row with
    probability p_noise.  A number in place of a pair fixes the value; snr_db=None: no noise.  No clamping: chain a PcmCodec for saturation.
    Every forward uses the next `draw` (fresh noise and parameters; a run is reproducible from `seed`); reset(draw) rewinds.  `row0`
    (forward's argument) numbers the first row, so that a batch cut into pieces draws what the whole batch would.  `last_stat`: the
    (rows, 4) tensor {g, s, mean square of x, snr_db or inf} of the last call.
    noise_grad "through": the noise level s, which follows the row's own RMS, takes part in the gradient | "detached": s is a constant, the
    gradient is g * dy.  CUDA tensors run the kernel; CPU tensors a numpy restatement of the same definition (forward only)."""

    def __init__(self, gain_db=(-6, 6), snr_db=(20, 40), p_noise=1.0, seed=0, noise_grad="through"):
        if noise_grad not in NOISE_GRAD_MODES:
            raise ValueError(f"noise_grad must be one of {NOISE_GRAD_MODES}, got {noise_grad!r}")
        if isinstance(p_noise, bool) or not isinstance(p_noise, (int, float)) or not 0.0 <= p_noise <= 1.0:
            raise ValueError(f"p_noise: expected a probability in [0, 1], got {p_noise!r}")
        super().__init__(seed)
        self.gain_db = _pair(gain_db, "gain_db")
        self.snr_db = None if snr_db is None else _pair(snr_db, "snr_db")
        self.p_noise = float(p_noise) if snr_db is not None else 0.0
        self.noise_grad = noise_grad
        self.last_stat = None

    @property
    def bounds(self):
        return (*self.gain_db, *(self.snr_db or (0.0, 0.0)), self.p_noise)

    def forward(self, x, row0=0):
        x = self._rows(x, row0)[0]
        draw = self._next_draw()
        if x.is_cuda:
            y, stat = dsp.DistortFn.apply(x.to(torch.float32), self.bounds, self.seed, draw, row0, self.noise_grad == "through")
        else:
            y, stat = self._host(x.detach().to(torch.float32), draw, row0)
        self.last_stat = stat
        return y

    def _host(self, x, draw, row0):
        return distort_rows_host(x, draw, row0, self.seed, self.bounds)

    def extra_repr(self):
        return (f"gain_db={self.gain_db}, snr_db={self.snr_db}, p_noise={self.p_noise}, seed={self.seed}, "
                f"noise_grad={self.noise_grad!r}")


class _LowpassFn(torch.autograd.Function):
    """y = F x, the zero-state biquad section; dx = F^T dy = flip(F(flip(dy))), the kernel's reverse launch"""

    @staticmethod
    def forward(ctx, x, coeffs):
        ctx.coeffs = coeffs
        return dsp.biquad(x, coeffs, clamp=False, mode="float")

    @staticmethod
    def backward(ctx, g):
        return dsp.biquad(g.contiguous(), ctx.coeffs, clamp=False, mode="float", reverse=True), None


class Lowpass(torch.nn.Module):
    """The RBJ biquad low-pass at `cutoff` Hz along the last axis of (B, 1, T), (C, N) or (N,), every row from a zero state; no clamp and
    no 16-bit grid (PcmCodec is the one with both).  CUDA: one launch of wm_biquad, differentiable through its adjoint; CPU: scipy's
    lfilter with the same float32 coefficients (forward only)."""

    def __init__(self, cutoff, sample_rate=SAMPLE_RATE):
        super().__init__()
        self.coeffs = dsp.biquad_lowpass_coeffs(sample_rate, cutoff)              # bad rates fail here
        self.cutoff, self.sample_rate = cutoff, sample_rate

    def forward(self, x):
        x = _time_rows(x, "x")
        if x.is_cuda:
            return _LowpassFn.apply(x.to(torch.float32), self.coeffs)
        from scipy.signal import lfilter
        b, a = np.array(self.coeffs[:3], dtype=np.float32), np.array((1.0,) + self.coeffs[3:], dtype=np.float32)
        y = lfilter(b, a, x.detach().to(torch.float32).numpy(), axis=-1)
        return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))

    def extra_repr(self):
        return f"cutoff={self.cutoff}, sample_rate={self.sample_rate}"


class Resampled(torch.nn.Module):
    """y = up(down(x))[..., :T] along the last axis of (B, 1, T), (C, N) or (N,), every row by itself: down is sample_rate -> rate, up is
    rate -> sample_rate, both the sinc resampler of dsp.resample_table (torchaudio's default design) without mixdown.  The output has the
    input's shape (ceil(sample_rate * ceil(rate * T / sample_rate) / rate) >= T: the cut is always possible); rate == sample_rate returns
    x.  CUDA: two launches of wm_resample_rows, differentiable through the same two launches with the transposed tables
    (dsp.ResampleRowsFn); CPU: the same float32 tables through F.conv1d, differentiable by autograd."""

    def __init__(self, rate, sample_rate=SAMPLE_RATE):
        super().__init__()
        dsp.resample_table(sample_rate, rate)                                     # bad rates fail here
        dsp.resample_table(rate, sample_rate)
        self.rate, self.sample_rate = int(rate), int(sample_rate)

    def forward(self, x):
        x = _time_rows(x, "x")
        if self.rate == self.sample_rate:
            return x
        T = x.shape[-1]
        rows = x.to(torch.float32).reshape(-1, T)
        if x.is_cuda:
            y = dsp.ResampleRowsFn.apply(dsp.ResampleRowsFn.apply(rows, self.sample_rate, self.rate), self.rate, self.sample_rate, T)
        else:
            from .inference import _resample_rows_host
            y = _resample_rows_host(_resample_rows_host(rows, self.sample_rate, self.rate), self.rate, self.sample_rate, T)
        return y.reshape(x.shape)

    def extra_repr(self):
        return f"rate={self.rate}, sample_rate={self.sample_rate}"


def code_entropy_kbps(codes, band, kcut, hop, sample_rate):
    """An ESTIMATE of the bitrate the int16 codes (rows, F, hop) of a TransformCodec call would cost: per band index (the `band`
    coefficients b * band .. below kcut) the first-order entropy H_b of the codes pooled over all rows and frames, band * H_b bits per frame,
    plus 8 bits per band per frame for the step; sample_rate / hop frames per second.  kbit/s per row-second.  No entropy coder is run and
    no real codec allocates bits this way: the figure relates snr_db to a bitrate, no more."""
    if codes.dim() != 3 or codes.shape[2] != hop or codes.numel() == 0:
        raise ValueError(f"codes: expected (rows, frames, {hop}) with at least one frame, got shape {tuple(codes.shape)}")
    nb = kcut // band
    sym = codes[:, :, :kcut].reshape(-1, nb, band).permute(1, 0, 2).reshape(nb, -1).to(torch.int64) + 32768     # (band index, pooled)
    per = sym.shape[1]
    keyed = (sym + 65536 * torch.arange(nb, device=sym.device).view(nb, 1)).reshape(-1)
    vals, counts = torch.unique(keyed, return_counts=True)
    p = counts.double() / per
    H = torch.zeros(nb, dtype=torch.float64, device=sym.device).index_add_(0, vals // 65536, -p * torch.log2(p))
    bits_per_frame = float((band * H + 8.0).sum())
    return bits_per_frame * sample_rate / hop / 1000.0


class TransformCodec(_RowDraws):
    """A STAND-IN for lossy compression on every row (clip or channel) of x, (B, 1, T), (C, N) or (N,): the signal path MP3 / AAC-like
    codecs share -- lapped MDCT at hop `hop`, per band of `band` coefficients a uniform quantiser whose step sits snr_db below the band's
    own level (noise shaped like the spectrum, weak coefficients fall into the dead zone; never finer than the 16-bit grid), an optional
    cut of everything above bandwidth_hz, synthesis with overlap-add (wm_mdct_codec in include/wm_hip.h has the definition).  It is not an
    MP3 or AAC encoder -- no psychoacoustic model, no bit reservoir, no entropy coder -- and PARITY WITH A REAL ENCODER IS UNMEASURED.
    snr_db: a number fixes the quality, a pair draws one value per row, reproducible from (seed, draw, row0 + r) (row_snr_db); 0..60.
    Every forward uses the next `draw`; reset(draw) rewinds; `row0` (forward's argument) numbers the first row, so that a batch cut into
    pieces draws what the whole batch would.  `last_snr_db`: the per-row values of the last call (a CPU tensor).
    grad "straight_through": the quantiser passes the gradient unchanged, the cut is kept | "dead_zone": coefficients coded 0 pass none
    (dsp.MdctCodecFn; the step's dependence on x is not differentiated).  CUDA tensors run the kernel, one launch each way; CPU tensors a
    float32 numpy restatement of the definition (forward only)."""

    def __init__(self, snr_db=(10, 30), bandwidth_hz=None, hop=256, band=8, sample_rate=SAMPLE_RATE, seed=0, grad="straight_through"):
        if grad not in dsp.MDCT_GRAD_MODES:
            raise ValueError(f"grad must be one of {dsp.MDCT_GRAD_MODES}, got {grad!r}")
        super().__init__(seed)
        self.snr_db = _pair(snr_db, "snr_db")
        if not 0.0 <= self.snr_db[0] <= self.snr_db[1] <= 60.0:
            raise ValueError(f"snr_db: expected values in [0, 60], got {snr_db!r}")
        self.kcut = dsp.mdct_kcut(hop, band, bandwidth_hz, sample_rate)           # bad hops, bands and bandwidths fail here
        self.hop, self.band, self.bandwidth_hz, self.sample_rate = hop, band, bandwidth_hz, sample_rate
        self.floor_step = dsp.mdct_default_floor_step(hop)
        self.grad = grad
        self.last_snr_db = None

    def _snr(self, x, row0):
        """x as time rows and the per-row quality of the CURRENT draw, which it does not advance"""
        x, _, numbers = self._rows(x, row0)
        return x, torch.from_numpy(row_snr_db(self.seed, self.draw, numbers, self.snr_db))

    def forward(self, x, row0=0):
        x, snr = self._snr(x, row0)
        self._next_draw()
        if x.is_cuda:
            y = dsp.MdctCodecFn.apply(x.to(torch.float32), snr.to(x.device), self.hop, self.band, self.kcut, self.floor_step, self.grad)
        else:
            y = self._host(x.detach().to(torch.float32), snr)[0]
        self.last_snr_db = snr
        return y

    def _host(self, x, snr):
        """(y, int16 codes (rows, F, hop)) of a CPU tensor"""
        return mdct_codec_rows_host(x, snr, self.hop, self.band, self.kcut, self.floor_step)

    @torch.no_grad()
    def estimate_kbps(self, x, row0=0):
        """An ESTIMATE of the bitrate this setting costs on x, in kbit/s per row-second: code_entropy_kbps of the codes the current draw
        gives (the draw is not advanced).  First-order entropy per band index plus 8 bits per band per frame for the step; no entropy
        coder is run.  It relates snr_db to a bitrate and says nothing about what an MP3 / AAC encoder would spend."""
        x, snr = self._snr(x, row0)
        if x.is_cuda:
            codes = dsp.mdct_codec(x.detach().to(torch.float32), snr.to(x.device), hop=self.hop, band=self.band, kcut=self.kcut,
                                   floor_step=self.floor_step, codes_out=True)[1]
        else:
            codes = self._host(x.detach().to(torch.float32), snr)[1]
        return code_entropy_kbps(codes, self.band, self.kcut, self.hop, self.sample_rate)

    def extra_repr(self):
        return (f"snr_db={self.snr_db}, bandwidth_hz={self.bandwidth_hz}, hop={self.hop}, band={self.band}, "
                f"sample_rate={self.sample_rate}, seed={self.seed}, grad={self.grad!r}")


class LpcCodec(_RowDraws):
    """A STAND-IN for a predictive speech codec on every row (clip or channel) of x, (B, 1, T), (C, N) or (N,): the signal path ADPCM, CELP,
    AMR-WB and SILK share -- per frame of `frame` samples an order-`order` linear predictor from the windowed autocorrelation, the
    prediction residual quantised by a uniform quantiser whose step sits snr_db below the residual's own level (never finer than the
    16-bit grid), all-pole synthesis, which shapes the white quantisation noise like the frame's spectral envelope (wm_lpc_codec in
    include/wm_hip.h has the definition).  It is not a speech codec -- open-loop quantisation, no LSP interpolation, no pitch
    predictor, no noise feedback, no entropy coder -- and PARITY WITH A REAL CODEC IS UNMEASURED, as is narrowband use behind
    Resampled(8000).  The output stays time-aligned with the input, so STOI applies.
    snr_db: a number fixes the quality, a pair draws one value per row, reproducible from (seed, draw, row0 + r) (row_lpc_snr_db); 0..60.
    Every forward uses the next `draw`; reset(draw) rewinds; `row0` (forward's argument) numbers the first row, so that a batch cut into
    pieces draws what the whole batch would.  `last_snr_db`: the per-row values of the last call (a CPU tensor).
    grad "straight_through": the gradient is dy itself (with the quantiser passed through, synthesis inverts the residual filter) |
    "dead_zone": residual samples coded 0 pass none -- the adjoint launch at the forward's coefficients (dsp.LpcCodecFn; the dependence of
    the coefficients and steps on x is not differentiated).  CUDA tensors run the kernel; CPU tensors a float32 numpy restatement of the
    definition (forward only)."""

    def __init__(self, snr_db=(10, 30), frame=320, order=16, sample_rate=SAMPLE_RATE, seed=0, grad="straight_through"):
        if grad not in dsp.LPC_GRAD_MODES:
            raise ValueError(f"grad must be one of {dsp.LPC_GRAD_MODES}, got {grad!r}")
        super().__init__(seed)
        self.snr_db = _pair(snr_db, "snr_db")
        if not 0.0 <= self.snr_db[0] <= self.snr_db[1] <= 60.0:
            raise ValueError(f"snr_db: expected values in [0, 60], got {snr_db!r}")
        dsp._lpc_dims(frame, order)
        dsp.lpc_tables(order, sample_rate)                                        # a bad sample rate fails here
        self.frame, self.order, self.sample_rate = frame, order, sample_rate
        self.floor_step = dsp.LPC_FLOOR_STEP
        self.grad = grad
        self.last_snr_db = None

    def forward(self, x, row0=0):
        x, rows, numbers = self._rows(x, row0)
        snr = torch.from_numpy(row_lpc_snr_db(self.seed, self.draw, numbers, self.snr_db))
        self._next_draw()
        if x.is_cuda:
            y = dsp.LpcCodecFn.apply(x.to(torch.float32), snr.to(x.device), self.frame, self.order, self.sample_rate, self.floor_step,
                                     self.grad)
        else:
            x32 = x.detach().to(torch.float32)
            y2 = _lpc_rows_host(x32.reshape(-1, x.shape[-1]).numpy(), snr.numpy(), self.frame, self.order, self.sample_rate,
                                self.floor_step)[0]
            y = torch.from_numpy(y2).reshape(x.shape)
        self.last_snr_db = snr
        return y

    def extra_repr(self):
        return (f"snr_db={self.snr_db}, frame={self.frame}, order={self.order}, sample_rate={self.sample_rate}, seed={self.seed}, "
                f"grad={self.grad!r}")


class NoiseSuppress(_RowDraws):
    """A STAND-IN for a single-channel noise suppressor on every row (clip or channel) of x, (B, 1, T), (C, N) or (N,) at 16 kHz: the
    signal path Ephraim-Malah / Scalart-Filho suppressors and WebRTC-style noise suppression share -- sine-windowed frames of 512 at hop
    256, a noise PSD per bin, a Wiener gain from a decision-directed a-priori SNR (weight `alpha`, over-subtraction `over`) floored at
    -reduce_db dB, synthesis with overlap-add (wm_noise_suppress in include/wm_hip.h has the definition).  It is the one attack here whose
    PURPOSE is to remove a low-level noise-like signal, which is what the watermark is.
    Its limits: it is a stand-in.  It uses one stationary noise estimate per row (the geometric mean of the row's own frame powers; or
    `noise_psd`, a (257,) or (rows, 257) profile, which is what an attacker who knows delta's average spectrum would pass).  It has no
    voice-activity detector, no minimum-statistics tracking and no neural denoiser.  A stationary tone counts as noise and is attenuated.
    The gradient holds the gains constant (the backward is the same launch on dy: suppress.NoiseSuppressFn).  PARITY WITH WebRTC NS,
    RNNoise, `noisereduce` OR ANY PRODUCT'S SUPPRESSOR IS UNMEASURED.  The output stays time-aligned, so STOI and NMR apply.
    reduce_db: a number fixes the depth, a pair draws one value per row, reproducible from (seed, draw, row0 + r) (row_reduce_db); 0..60.
    Every forward uses the next `draw`; reset(draw) rewinds; `row0` (forward's argument) numbers the first row, so that a batch cut into
    pieces draws what the whole batch would.  `last_reduce_db`: the per-row values of the last call (a CPU tensor).
    CUDA tensors run the kernels; CPU tensors a float64 numpy restatement of the definition, rounded once (forward only)."""

    def __init__(self, reduce_db=(6, 24), over=1.0, alpha=0.98, noise_psd=None, seed=0):
        super().__init__(seed)
        self.reduce_db = _pair(reduce_db, "reduce_db")
        if not 0.0 <= self.reduce_db[0] <= self.reduce_db[1] <= suppress.SUPPRESS_MAX_REDUCE_DB:
            raise ValueError(f"reduce_db: expected values in [0, 60], got {reduce_db!r}")
        self.alpha, self.over = suppress._chk_scalars(alpha, over)
        if noise_psd is not None:
            if not isinstance(noise_psd, torch.Tensor) or noise_psd.dim() not in (1, 2) or noise_psd.shape[-1] != suppress.SUPPRESS_BINS:
                raise ValueError(f"noise_psd: expected None or a (257,) or (rows, 257) tensor, got "
                                 f"{tuple(noise_psd.shape) if isinstance(noise_psd, torch.Tensor) else type(noise_psd).__name__}")
            suppress._profile_rows(noise_psd, noise_psd.numel() // suppress.SUPPRESS_BINS, noise_psd.device)      # non-finite or negative values fail here
            noise_psd = noise_psd.detach().to(torch.float32).contiguous()
        self.register_buffer("noise_psd", noise_psd)
        self.last_reduce_db = None

    def forward(self, x, row0=0):
        x, rows, numbers = self._rows(x, row0)
        x32 = x.to(torch.float32)
        x2 = x32.reshape(rows, x.shape[-1])
        prof = suppress._profile_rows(self.noise_psd, rows, x.device)            # a profile for another number of rows fails here
        rd = torch.from_numpy(row_reduce_db(self.seed, self.draw, numbers, self.reduce_db))
        self._next_draw()
        if x.is_cuda:
            y = suppress.NoiseSuppressFn.apply(x2, rd.to(x.device), prof, self.alpha, self.over)
        else:
            y = suppress.suppress_rows_host(x2, rd, None, prof, self.alpha, self.over)
        self.last_reduce_db = rd
        return y.reshape(x.shape)

    def extra_repr(self):
        prof = None if self.noise_psd is None else tuple(self.noise_psd.shape)
        return f"reduce_db={self.reduce_db}, over={self.over}, alpha={self.alpha}, noise_psd={prof}, seed={self.seed}"


def echo_ir(delay_s, gain_db, sample_rate=SAMPLE_RATE):
    """The response of one echo `delay_s` seconds behind the direct sound and gain_db against it, at unit energy:
    {1, 0, ..., 0, g} / sqrt(1 + g^2) with g = 10^(gain_db / 20) at tap round(delay_s * sample_rate).  A float32 tensor for Convolved."""
    for v, name in ((delay_s, "delay_s"), (gain_db, "gain_db"), (sample_rate, "sample_rate")):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    if sample_rate <= 0:
        raise ValueError(f"sample_rate must be positive, got {sample_rate!r}")
    d = int(round(delay_s * sample_rate))
    if not 1 <= d < dsp.FIR_MAX_TAPS:
        raise ValueError(f"delay_s: the echo must fall on a tap in [1, {dsp.FIR_MAX_TAPS - 1}], got tap {d} ({delay_s!r} s at {sample_rate} Hz)")
    g = 10.0 ** (gain_db / 20.0)
    h = torch.zeros(d + 1, dtype=torch.float64)
    h[0], h[d] = 1.0 / math.sqrt(1.0 + g * g), g / math.sqrt(1.0 + g * g)
    return h.to(torch.float32)


class Convolved(_RowDraws):
    """y = h * x, causal and cut to the input's length, for every row (clip or channel) of x, (B, 1, T), (C, N) or (N,): lag 0 stays at
    lag 0, so per-sample labels stay aligned.  h: a (K,) impulse response for all rows, or an (R, K) bank of (measured) responses, of which
    row r takes entry floor(u * R), u drawn from (seed, draw, row0 + r) (row_bank_index); K <= 16384.  normalize: every response is
    scaled to unit energy first (a response of zero energy is refused).  Every forward uses the next `draw`; reset(draw) rewinds; `row0`
    (forward's argument) numbers the first row, so that a batch cut into pieces draws what the whole batch would.  `last_index`: the bank
    entries of the last call (a CPU tensor; None without a bank).  h is a constant: no gradient flows to it.
    CUDA tensors run wm_fir_rows, one launch each way (dsp.FirRowsFn); CPU tensors F.conv1d in float32, differentiable by autograd."""

    def __init__(self, h, normalize=False, seed=0):
        if not isinstance(h, torch.Tensor) or h.dim() not in (1, 2) or h.numel() == 0 or not 1 <= h.shape[-1] <= dsp.FIR_MAX_TAPS:
            raise ValueError(f"h: expected a (K,) or (R, K) tensor with 1 <= K <= {dsp.FIR_MAX_TAPS}, got "
                             f"{tuple(h.shape) if isinstance(h, torch.Tensor) else type(h).__name__}")
        if not isinstance(normalize, bool):
            raise ValueError(f"normalize: expected a bool, got {normalize!r}")
        super().__init__(seed)
        h = h.detach().to(torch.float64)
        if not bool(torch.isfinite(h).all()):
            raise ValueError("h: expected finite taps")
        if normalize:
            energy = h.pow(2).sum(dim=-1, keepdim=True)
            if not bool((energy > 0).all()):
                raise ValueError("h: a response of zero energy cannot be normalised")
            h = h / energy.sqrt()
        self.register_buffer("h", h.to(torch.float32).contiguous())
        self.normalize = normalize
        self.last_index = None

    def forward(self, x, row0=0):
        x, rows, numbers = self._rows(x, row0)
        draw = self._next_draw()
        h = self.h if self.h.device == x.device else self.h.to(x.device)
        self.last_index = None
        if h.dim() == 2:
            self.last_index = torch.from_numpy(row_bank_index(self.seed, draw, numbers, h.shape[0]))
            h = h[self.last_index.to(x.device)]                                   # gathered on the device: per-row taps
        x32 = x.to(torch.float32)
        if x.is_cuda:
            return dsp.FirRowsFn.apply(x32.reshape(rows, -1), h).reshape(x.shape)
        return _conv_rows_host(x32.reshape(rows, -1), h).reshape(x.shape)

    def extra_repr(self):
        return f"h={tuple(self.h.shape)}, normalize={self.normalize}, seed={self.seed}"


class Reverb(_RowDraws):
    """Synthetic reverberation on every row (clip or channel) of x, (B, 1, T), (C, N) or (N,): the row convolved (causal, cut to the
    input's length, lag 0 at lag 0) with a response of `taps` samples drawn for it -- a direct tap followed by Gaussian noise whose
    amplitude falls 60 dB in rt60 seconds, at a direct-to-reverberant energy ratio of drr_db and unit total energy (wm_rir_synth in
    include/wm_hip.h has the definition; rir_taps restates it).  It is NOT a room simulation -- no geometry, no early reflections, no
    frequency-dependent decay -- and A WATERMARK'S SURVIVAL IN REAL ROOMS IS UNMEASURED; measured responses go through Convolved.
    rt60, drr_db: a number fixes the value, a pair draws one per row, reproducible from (seed, draw, row0 + r) (row_reverb_params).
    Every forward uses the next `draw` (fresh parameters and responses); reset(draw) rewinds; `row0` (forward's argument) numbers the
    first row, so that a batch cut into pieces draws what the whole batch would.  `last_params`: the (rows, 2) {rt60, drr_db} of the last
    call (a CPU tensor); `last_ir`: its (rows, taps) responses (on x's device).  The responses are constants of the graph.
    CUDA tensors run wm_rir_synth and wm_fir_rows (dsp.FirRowsFn, one launch each way); CPU tensors rir_taps and F.conv1d in float32,
    differentiable by autograd."""

    def __init__(self, rt60=(0.1, 0.4), drr_db=(0, 12), taps=2048, sample_rate=SAMPLE_RATE, seed=0):
        super().__init__(seed)
        self.rt60, self.drr_db = _pair(rt60, "rt60"), _pair(drr_db, "drr_db")
        if not self.rt60[0] > 0.0:
            raise ValueError(f"rt60: expected positive values, got {rt60!r}")
        self.taps = _chk_int(taps, "taps", 1, dsp.FIR_MAX_TAPS)
        self.sample_rate = _chk_positive(sample_rate, "sample_rate")
        self.last_params = self.last_ir = None

    def forward(self, x, row0=0):
        x, rows, numbers = self._rows(x, row0)
        draw = self._next_draw()
        rt60, drr = row_reverb_params(self.seed, draw, numbers, self.rt60, self.drr_db)
        self.last_params = torch.from_numpy(np.stack([rt60, drr], axis=1))
        x32 = x.to(torch.float32)
        if x.is_cuda:
            h = dsp.rir_synth(self.last_params.to(x.device), self.taps, self.sample_rate, self.seed, draw, row0)
            y = dsp.FirRowsFn.apply(x32.reshape(rows, -1), h)
        else:
            h = torch.from_numpy(np.stack([rir_taps(self.seed, draw, row0 + r, rt60[r], drr[r], self.taps, self.sample_rate)
                                           for r in range(rows)]).astype(np.float32))
            y = _conv_rows_host(x32.reshape(rows, -1), h)
        self.last_ir = h
        return y.reshape(x.shape)

    def extra_repr(self):
        return f"rt60={self.rt60}, drr_db={self.drr_db}, taps={self.taps}, sample_rate={self.sample_rate}, seed={self.seed}"


class TimeWarp(_RowDraws):
    """The desynchronising channel on every row (clip or channel) of x, (B, 1, T), (C, N) or (N,): y[t] reads x at the position
    p(t) = speed * t + shift + flutter, through a Hann-windowed sinc interpolator of `zeros` zero crossings a side whose cutoff follows the
    speed, so a faster playback does not alias (wm_time_warp in include/wm_hip.h has the definition).  It is a speed change -- tempo and
    pitch move together, as on a turntable or with a wrong clock --, plus sinusoidal wow / flutter, plus a cut of shift_s seconds at the
    front (negative: silence in front).  The pitch-preserving stretch is TimeStretch (WSOLA) and the pitch shift at constant tempo is
    PitchShift; a phase vocoder is not built, and A WATERMARK'S SURVIVAL AGAINST REAL PLAYERS AND TAPES IS UNMEASURED.
    THE OUTPUT KEEPS THE INPUT'S LENGTH AND THE LABELS ARE NOT MOVED: where the read position leaves the row the output is silence, and that
    silence -- like every warped sample -- is still labelled as its clip is; a per-sample localisation label stays at its output index.
    speed in [0.5, 2], shift_s, flutter_hz in (0, sample_rate / 4], flutter_depth in [0, 0.25] (the relative peak deviation of the
    instantaneous speed, which keeps p strictly increasing and the cutoff at 0.4 or more): a number fixes the value, a pair draws one per
    row, reproducible from (seed, draw, row0 + r) (row_warp_params); the two flutter arguments are given together or not at all.
    Every forward uses the next `draw`; reset(draw) rewinds; `row0` (forward's argument) numbers the first row, so that a batch cut into
    pieces draws what the whole batch would.  `last_params`: the (rows, 6) {a, off, d, w, phi, c} of the last call (a CPU tensor).  The
    parameters are constants of the graph.  There is no shortcut for speed 1: the kernel hands a whole-sample shift on bit for bit.
    CUDA tensors run wm_time_warp, one launch each way (dsp.TimeWarpFn); CPU tensors the same definition in torch ops (gathered taps times
    float32 weights), differentiable by autograd."""

    RES = 512

    def __init__(self, speed=(0.9, 1.1), shift_s=0.0, flutter_hz=None, flutter_depth=None, zeros=16, sample_rate=SAMPLE_RATE, seed=0):
        super().__init__(seed)
        self.sample_rate = _chk_positive(sample_rate, "sample_rate")
        self.speed, self.shift_s = _pair(speed, "speed"), _pair(shift_s, "shift_s")
        if not 0.5 <= self.speed[0] <= self.speed[1] <= 2.0:
            raise ValueError(f"speed: expected values in [0.5, 2], got {speed!r}")
        if (flutter_hz is None) != (flutter_depth is None):
            raise ValueError("flutter_hz and flutter_depth: give both or neither")
        self.flutter_hz = None if flutter_hz is None else _pair(flutter_hz, "flutter_hz")
        self.flutter_depth = None if flutter_depth is None else _pair(flutter_depth, "flutter_depth")
        if self.flutter_hz is not None:
            if not 0.0 < self.flutter_hz[0] <= self.flutter_hz[1] <= sample_rate / 4:
                raise ValueError(f"flutter_hz: expected values in (0, sample_rate / 4 = {sample_rate / 4}], got {flutter_hz!r}")
            if not 0.0 <= self.flutter_depth[0] <= self.flutter_depth[1] <= 0.25:
                raise ValueError(f"flutter_depth: expected values in [0, 0.25], got {flutter_depth!r}")
        dsp.time_warp_table(zeros, self.RES)                                      # a bad `zeros` fails here
        self.zeros = zeros
        self.last_params = None

    def forward(self, x, row0=0):
        x, rows, numbers = self._rows(x, row0)
        draw = self._next_draw()
        self.last_params = torch.from_numpy(row_warp_params(self.seed, draw, numbers, self.speed, self.shift_s,
                                                            self.flutter_hz, self.flutter_depth, self.sample_rate))
        x2 = x.to(torch.float32).reshape(rows, -1)
        if x.is_cuda:
            y = dsp.TimeWarpFn.apply(x2, self.last_params.to(x.device), dsp._time_warp_table_on(self.zeros, self.RES, x.device),
                                     self.zeros, self.RES)
        else:
            y = _warp_rows_host(x2, self.last_params, dsp.time_warp_table(self.zeros, self.RES), self.zeros, self.RES)
        return y.reshape(x.shape)

    def extra_repr(self):
        return (f"speed={self.speed}, shift_s={self.shift_s}, flutter_hz={self.flutter_hz}, flutter_depth={self.flutter_depth}, "
                f"zeros={self.zeros}, sample_rate={self.sample_rate}, seed={self.seed}")


class _Wsola(_RowDraws):
    """What TimeStretch and PitchShift share: the frame and the search range"""

    def __init__(self, frame, search, seed):
        super().__init__(seed)
        dsp._wsola_dims(frame, search)
        self.frame, self.search = frame, search
        self.last_params = self.last_delta = None

    def _stretch(self, x2, rates, n_out):
        """(rows, n) -> (rows, n_out) at the float32 rates; keeps the offsets in last_delta (on x2's device)"""
        if x2.is_cuda:
            y, delta = dsp.WsolaFn.apply(x2, torch.from_numpy(rates).to(x2.device), n_out, self.frame, self.search)
        else:
            y, delta = _wsola_rows_host(x2, rates, n_out, self.frame, self.search)
        self.last_delta = delta
        return y


class TimeStretch(_Wsola):
    """A pitch-preserving change of tempo on every row (clip or channel) of x, (B, 1, T), (C, N) or (N,), by waveform-similarity
    overlap-add (WSOLA; wm_wsola in include/wm_hip.h has the definition): frames of `frame` samples are copied from the input to places
    frame / 2 apart in the output, each taken within `search` samples of its nominal place rate * t where it continues its predecessor
    best, and cross-faded over half a frame.  The spectrum stays and the time axis moves: the attack a per-sample detector is least
    prepared for.  A stretch is a PIECEWISE COPY WITH CROSS-FADED JUMPS: the search is rectangular, there is no transient detection,
    PARITY WITH ANY REAL EDITOR'S STRETCH IS UNMEASURED, and STOI under it says nothing.
    THE OUTPUT KEEPS THE INPUT'S LENGTH AND THE LABELS ARE NOT MOVED (TimeWarp's contract): at rate > 1 the input runs out and the rest is
    silence, at rate < 1 the end of the input is not reached; every sample is still labelled as its clip is.
    rate in [0.5, 2], input samples consumed per output sample (above 1 plays faster): a number fixes it, a pair draws one per row,
    reproducible from (seed, draw, row0 + r) (row_stretch_rates).  Every forward uses the next `draw`; reset(draw) rewinds; `row0`
    numbers the first row, so that a batch cut into pieces draws what the whole batch would.  `last_params`: the (rows,) float32 rates of
    the last call (a CPU tensor); `last_delta`: its (rows, K) int32 offsets, where they were computed.  The chosen positions are constants
    of the graph: the gradient is that of the linear gather.  At rate 1 the output is the input bit for bit.
    CUDA tensors run wm_wsola, one launch each way (dsp.WsolaFn); CPU tensors the same definition in torch ops, differentiable by autograd."""

    def __init__(self, rate=(0.9, 1.1), frame=512, search=128, seed=0):
        super().__init__(frame, search, seed)
        self.rate = _pair(rate, "rate")
        if not 0.5 <= self.rate[0] <= self.rate[1] <= 2.0:
            raise ValueError(f"rate: expected values in [0.5, 2], got {rate!r}")

    def forward(self, x, row0=0):
        x, rows, numbers = self._rows(x, row0)
        draw = self._next_draw()
        rates = row_stretch_rates(self.seed, draw, numbers, self.rate)
        self.last_params = torch.from_numpy(rates)
        x2 = x.to(torch.float32).reshape(rows, -1)
        return self._stretch(x2, rates, x2.shape[1]).reshape(x.shape)

    def extra_repr(self):
        return f"rate={self.rate}, frame={self.frame}, search={self.search}, seed={self.seed}"


class PitchShift(_Wsola):
    """A change of pitch at constant tempo on every row of x, (B, 1, T), (C, N) or (N,): a TimeStretch that makes the row longer by the
    factor beta = 2^(semitones / 12), played back beta times as fast through TimeWarp's interpolator, so the duration is the input's and
    every frequency is multiplied by beta.  No second kernel: wm_wsola at rate float32(1 / beta) to m = max(n, ceil(beta n)) samples (a
    row's samples past its own m are silence), wm_time_warp on these with {a = beta, off = 0, d = 0, w = 0, phi = 0, c = min(1, 1 /
    beta)}, the first n samples.  TimeStretch's limits hold -- a piecewise copy with cross-faded jumps, PARITY WITH ANY REAL EDITOR'S
    PITCH SHIFT IS UNMEASURED -- and formants move with the pitch.  The output keeps the input's length and the labels are not moved.
    semitones in [-12, 12]: a number fixes it, a pair draws one per row from (seed, draw, row0 + r) (row_pitch_params).  `last_params`: the
    (rows, 3) float32 {semitones, beta, rate} of the last call (a CPU tensor); `last_delta`: the stretch's offsets.  seed, draw, reset and
    row0 as in TimeStretch.  CUDA tensors run the two launches (dsp.WsolaFn, dsp.TimeWarpFn), CPU tensors the same definitions in torch
    ops, differentiable by autograd."""

    RES = TimeWarp.RES

    def __init__(self, semitones=(-1, 1), frame=512, search=128, zeros=16, seed=0):
        super().__init__(frame, search, seed)
        self.semitones = _pair(semitones, "semitones")
        if not -12.0 <= self.semitones[0] <= self.semitones[1] <= 12.0:
            raise ValueError(f"semitones: expected values in [-12, 12], got {semitones!r}")
        dsp.time_warp_table(zeros, self.RES)                                      # a bad `zeros` fails here
        self.zeros = zeros

    def forward(self, x, row0=0):
        x, rows, numbers = self._rows(x, row0)
        draw = self._next_draw()
        st, beta, rates = row_pitch_params(self.seed, draw, numbers, self.semitones)
        self.last_params = torch.from_numpy(np.stack([st, beta, rates], axis=1))
        x2 = x.to(torch.float32).reshape(rows, -1)
        n = x2.shape[1]
        m = np.maximum(n, np.ceil(beta.astype(np.float64) * n)).astype(np.int64)
        z = self._stretch(x2, rates, int(m.max()))
        past = torch.arange(z.shape[1])[None, :] >= torch.from_numpy(m)[:, None]
        if bool(past.any()):
            z = z.masked_fill(past.to(z.device), 0.0)                             # every row ends at its own m
        b64 = beta.astype(np.float64)
        params = torch.from_numpy(np.stack([b64, 0 * b64, 0 * b64, 0 * b64, 0 * b64, np.minimum(1.0, 1.0 / b64)], axis=1).astype(np.float32))
        if x.is_cuda:
            y = dsp.TimeWarpFn.apply(z, params.to(x.device), dsp._time_warp_table_on(self.zeros, self.RES, x.device), self.zeros, self.RES)
        else:
            y = _warp_rows_host(z, params, dsp.time_warp_table(self.zeros, self.RES), self.zeros, self.RES)
        return y[:, :n].reshape(x.shape)

    def extra_repr(self):
        return f"semitones={self.semitones}, frame={self.frame}, search={self.search}, zeros={self.zeros}, seed={self.seed}"


class Splice(_RowDraws):
    """The editing attack on every row (clip or channel) of a watermarked signal, (B, 1, T), (C, N) or (N,): up to max_spans spans per row,
    each present with probability p_span, of a length drawn uniformly from length_s (seconds; a number fixes it) at a uniform position, are
    cut out and replaced -- with probabilities kinds = (original, silence, moved) -- by the same span of the CLEAN signal, by silence, or by
    clean audio from elsewhere in the same row (a circular shift by 1 .. n - 1 samples).  Where spans overlap the later one wins.
    forward(watermarked, clean, row0=0) returns (tampered, labels): tampered has the input's shape, labels is the (rows, ceil(n / 32)) int32
    bit mask "this sample is still watermarked" (bit j of word w is sample 32 w + j, tail bits zero; unpack_labels gives booleans).
    IT TAKES TWO INPUTS: it is not a `codec=` and does not go into torch.nn.Sequential chains; it is the `tamper=` argument of
    forward_losses / train_step / eval_forward / evaluate_batches and evaluate_localization, where it comes last, behind any codec, so the
    labels are exact whatever the codec did to the time axis.
    Limits: the cuts are rectangular, with no crossfade; "moved" audio comes from the same row only; a span longer than the row is cut to
    the row's length; WHETHER A MODEL TRAINED WITH IT LOCALISES REAL EDITS IS UNMEASURED.
    Every forward uses the next `draw`; reset(draw) rewinds; `row0` numbers the first row, so that a batch cut into pieces draws what the
    whole batch would (row_splice_spans restates the draw).  `last_labels`: the labels of the last call.  The gradient reaches
    `watermarked` where the label is 1; `clean` is data.  CUDA tensors run wm_splice, one launch each way (dsp.SpliceFn); CPU tensors
    splice_rows_host (forward only)."""

    def __init__(self, max_spans=2, p_span=0.5, length_s=(0.05, 0.4), kinds=(1 / 3, 1 / 3, 1 / 3), seed=0, sample_rate=SAMPLE_RATE):
        super().__init__(seed)
        _chk_int(max_spans, "max_spans", 1, dsp.SPLICE_MAX_SPANS)
        if isinstance(p_span, bool) or not isinstance(p_span, (int, float)) or not 0.0 <= p_span <= 1.0:
            raise ValueError(f"p_span: expected a probability in [0, 1], got {p_span!r}")
        _chk_positive(sample_rate, "sample_rate")
        self.length_s = _pair(length_s, "length_s")
        if not self.length_s[0] > 0.0:
            raise ValueError(f"length_s: expected positive lengths, got {length_s!r}")
        if (not isinstance(kinds, (tuple, list)) or len(kinds) != 3 or
                not all(isinstance(k, (int, float)) and not isinstance(k, bool) and 0.0 <= k <= 1.0 for k in kinds) or
                abs(sum(kinds) - 1.0) > 1e-6):
            raise ValueError(f"kinds: expected three probabilities (original, silence, moved) that sum to 1, got {kinds!r}")
        self.max_spans, self.p_span, self.kinds, self.sample_rate = max_spans, float(p_span), tuple(map(float, kinds)), sample_rate
        self.len_lo = max(1, int(round(self.length_s[0] * sample_rate)))
        self.len_hi = max(self.len_lo, int(round(self.length_s[1] * sample_rate)))
        if self.len_hi > dsp.SPLICE_MAX_N:
            raise ValueError(f"length_s: {self.length_s[1]} s is more than the 2^24 samples a row may have")
        # the kernel takes float32 probabilities and wants p_original + p_silence <= 1 of THOSE: step p_silence down where rounding broke it
        po, ps = np.float32(self.kinds[0]), np.float32(self.kinds[1])
        while float(po) + float(ps) > 1.0:
            ps = np.nextafter(ps, np.float32(0.0))
        self.p_original, self.p_silence = float(po), float(ps)
        self.last_labels = None

    def cut(self, n):
        """wm_splice's scalars for rows of n samples, row_splice_spans's keywords: the span lengths never exceed the row"""
        hi = min(self.len_hi, int(n))
        return dict(max_spans=self.max_spans, p_span=self.p_span, len_lo=min(self.len_lo, hi), len_hi=hi, p_original=self.p_original,
                    p_silence=self.p_silence)

    def forward(self, watermarked, clean, row0=0):
        a, rows, _ = self._rows(watermarked, row0)
        b = _time_rows(clean, "clean")
        if a.shape != b.shape or a.device != b.device:
            raise ValueError(f"watermarked and clean: expected equal shapes on one device, got {tuple(a.shape)} on {a.device} and "
                             f"{tuple(b.shape)} on {b.device}")
        n = a.shape[-1]
        if n > dsp.SPLICE_MAX_N:
            raise ValueError(f"a row may have 2^24 samples, got {n}")
        draw = self._next_draw()
        cut = self.cut(n)
        if a.is_cuda:
            y, lab = dsp.SpliceFn.apply(a.to(torch.float32).contiguous(), b.detach().to(torch.float32).contiguous(),
                                        tuple(cut[k] for k in ("max_spans", "p_span", "len_lo", "len_hi", "p_original", "p_silence")),
                                        self.seed, draw, row0)
        else:
            y, labels = splice_rows_host(a.detach().to(torch.float32).reshape(rows, n).numpy(),
                                         b.detach().to(torch.float32).reshape(rows, n).numpy(), self.seed, draw, row0, **cut)
            y, lab = torch.from_numpy(y).reshape(a.shape), torch.from_numpy(pack_labels(labels).view(np.int32))
        self.last_labels = lab
        return y, lab

    def extra_repr(self):
        return (f"max_spans={self.max_spans}, p_span={self.p_span}, length_s={self.length_s}, kinds={self.kinds}, seed={self.seed}, "
                f"sample_rate={self.sample_rate}")


def _ratio(num, den):
    return num / den if den else math.nan


def localization_metrics(tampered_counts, clean_counts):
    """evaluate_localization's ratios from the pooled integer counts (tp, fp, fn, tn) of the tampered watermarked half and of the clean
    half; a ratio with a zero denominator is NaN"""
    tp, fp, fn, tn = (int(v) for v in tampered_counts)
    _, cfp, _, ctn = (int(v) for v in clean_counts)
    total = tp + fp + fn + tn
    return OrderedDict(iou=_ratio(tp, tp + fp + fn), precision=_ratio(tp, tp + fp), recall=_ratio(tp, tp + fn),
                       sample_accuracy=_ratio(tp + tn, total), clean_false_positive_rate=_ratio(cfp, cfp + ctn),
                       watermarked_fraction=_ratio(tp + fn, total))


@torch.no_grad()
def evaluate_localization(generator, detector, batches, tamper, device="cuda", message_bits=16, messages=None, threshold=0.5, codec=None):
    """Does the per-sample track localise?  Every batch s is watermarked (s_w = s + delta, or codec(s + delta)), tampered (s_t, labels =
    tamper(s_w, s), a Splice), and the Detector runs on cat([s_t, s]); its prediction sigmoid(logits[:, :, 0]) > threshold is scored against
    the labels by dsp.loc_counts -- integer counts per row on the device, pooled over all batches.  Eval mode, no_grad.  Returns
      iou = tp / (tp + fp + fn), precision, recall, sample_accuracy     over the tampered watermarked half ("positive" = still watermarked)
      clean_false_positive_rate = fp / (fp + tn)                         over the clean half, whose labels are all 0
      watermarked_fraction                                               the share of label 1 in the tampered half
      bit_accuracy    per clip, every bit decoded as the majority of sigmoid > 0.5 over the samples WITH LABEL 1 only, against the message;
                      clips without such a sample are left out
      rows            the clips pooled.
    A ratio with a zero denominator is NaN.  `messages` (optional list, one tensor per batch) replaces the random draw.  What this
    measures is agreement with Splice's rectangular cuts; it says nothing about edits made with a crossfade or by another tool."""
    if not isinstance(tamper, Splice):
        raise TypeError(f"tamper: expected an attacks.Splice, got {type(tamper).__name__}")
    generator.eval(); detector.eval()
    pooled = torch.zeros(2, 4, dtype=torch.int64, device=device)
    bit_acc, rows = [], 0
    for bi, s in enumerate(batches):
        s = s.to(device)
        B, T = s.shape[0], s.shape[-1]
        message = (messages[bi].to(device) if messages is not None else
                   torch.randint(0, 2 ** message_bits, (B,), device=device))
        s_w = s + postprocess(generator(s, message))
        if codec is not None:
            s_w = codec(s_w)
        s_t, labels = tamper(s_w, s)
        logits = detector(torch.cat([s_t, s], dim=0))
        counts = dsp.loc_counts(logits, labels, threshold).to(torch.int64)
        pooled += torch.stack([counts[:B].sum(dim=0), counts[B:].sum(dim=0)])
        rows += B
        nbits = logits.shape[-1] - 1
        if nbits > 0:
            keep = ((labels[:, :, None] >> torch.arange(32, device=labels.device, dtype=torch.int32)) & 1).reshape(B, -1)[:, :T].bool()
            n1 = keep.sum(dim=1)
            votes = ((logits[:B, :, 1:] > 0) & keep[:, :, None]).sum(dim=1)                      # sigmoid(x) > 0.5 is x > 0
            decoded = 2 * votes > n1[:, None]
            bits = ((message.unsqueeze(1) & (1 << torch.arange(nbits, device=logits.device))) > 0)
            bit_acc.append((decoded == bits).float().mean(dim=1)[n1 > 0])
    pooled = pooled.cpu().tolist()
    res = localization_metrics(pooled[0], pooled[1])
    acc = torch.cat(bit_acc) if bit_acc else torch.empty(0)
    res["bit_accuracy"] = float(acc.double().mean()) if acc.numel() else math.nan
    res["rows"] = rows
    return res


@torch.no_grad()
def evaluate_robustness(generator, detector, batches, attacks, device="cuda", message_bits=16, messages=None, quality=()):
    """How detection moves under distortions: {name: {"watermarked_prob", "clean_prob", "bit_accuracy", "delta_rms"}} for every entry of
    `attacks` (name -> module on (B, 1, T)) and for "none", the undistorted signal.  Eval mode, no_grad; the Generator runs once per batch,
    every attack is applied to BOTH s + delta and s (the false-positive side: what an attack does to clean audio is half of the answer),
    as one call on their concatenation, and the Detector runs once per attack on the result.  The per-batch reductions are eval_forward's
    and the per-clip values of all batches are pooled and averaged once, as evaluate_batches does (a ragged last batch weighs by its
    clips).  `messages` (optional list, one tensor per batch) replaces the random draw.
    `quality=("stoi",)` adds what the attack does to the speech itself, three more keys in every row ("none" included), from ONE
    dsp.stoi call per attack on the same 2B rows against the clean s: "stoi" (the attacked watermarked half), "stoi_attack_only" (the
    attacked clean half: the gap between the two is what the watermark adds under that attack) and "stoi_rows", the clips pooled --
    clips with fewer than 30 spectral frames have no score and are left out, not averaged in as the sentinel 1e-5 (NaN when none is
    left).  STOI assumes time-aligned signals: under TimeWarp it is low by construction and says nothing.  The default, quality=(), is
    the call as it was.
    `"nmr"` in quality adds five keys per row from ONE masking.masking call per attack on the same 2B rows against cat([s, s]): "nmr_db" and
    "nmr_db_attack_only" (the mean over the pooled clips of the noise-to-mask ratio in dB of the attacked watermarked / attacked clean half),
    "audible_share" and "audible_share_attack_only" (audible cells / cells over the pooled clips) and "nmr_rows", the clips pooled: those with
    a frame (cells > 0) and a score that is not NaN in either half.  The clean half of "none" is s against s: -inf and share 0, reported as
    such.  One simultaneous-masking model at an assumed playback level (see masking.py for the limits); like STOI it assumes time-aligned
    signals, so under TimeWarp, TimeStretch and PitchShift the number is meaningless."""
    return _evaluate_robustness(generator, detector, batches, attacks, device, message_bits, messages, quality, False)


@torch.no_grad()
def evaluate_robustness_by_class(generator, detector, batches, attacks, device="cuda", message_bits=16, messages=None, quality=()):
    """evaluate_robustness with every number given again per class of clean clip: each row gains "by_class", {"speech" | "noise" |
    "silent": {"clips": count, and the row's keys over that class's clips (NaN for an empty class)}}.  The classes are
    curate.clip_classes of the clean batch -- one wm_clip_features launch per batch, before the attacks -- and a clip with a non-finite
    sample is in none.  With quality=("stoi",) a class's "stoi_rows" counts its scored clips.  (evaluate_robustness keeps its parameter
    list, so the per-class report is a call of its own rather than a by_class argument.)"""
    return _evaluate_robustness(generator, detector, batches, attacks, device, message_bits, messages, quality, True)


def _nmr_pool(parts, pick=None):
    """the five "nmr" keys of one row of evaluate_robustness from the per-clip CPU tensors (nmr wm, nmr clean, audible wm, audible clean,
    cells), over the clips of `pick` (all by default) that have a frame and a score in both halves"""
    nw, nc, aw, ac, cells = parts
    ok = (cells > 0) & ~torch.isnan(nw) & ~torch.isnan(nc)
    if pick is not None:
        ok = ok & pick
    rows, total = int(ok.sum()), int(cells[ok].sum())
    if rows == 0:
        return {"nmr_db": math.nan, "nmr_db_attack_only": math.nan, "audible_share": math.nan, "audible_share_attack_only": math.nan,
                "nmr_rows": 0}
    return {"nmr_db": float(nw[ok].double().mean()), "nmr_db_attack_only": float(nc[ok].double().mean()),
            "audible_share": int(aw[ok].sum()) / total, "audible_share_attack_only": int(ac[ok].sum()) / total, "nmr_rows": rows}


def _evaluate_robustness(generator, detector, batches, attacks, device, message_bits, messages, quality, by_class):
    """the loop of evaluate_robustness and evaluate_robustness_by_class"""
    from .step import _eval_reductions
    from .quality import check_metrics
    quality = check_metrics(quality)
    if "none" in attacks:
        raise ValueError('attacks: the name "none" is taken by the undistorted row')
    generator.eval(); detector.eval()
    keys = {"watermarked_prob": "prob_watermarked", "clean_prob": "prob_clean", "bit_accuracy": "bit_accuracy",
            "delta_rms": "delta_rms"}
    named = [("none", None)] + list(attacks.items())
    acc = OrderedDict((name, {k: [] for k in keys}) for name, _ in named)
    stoi_acc = OrderedDict((name, ([], [])) for name, _ in named)
    stoi_all = OrderedDict((name, ([], [], [])) for name, _ in named)               # by_class: both halves unmasked, and the mask
    nmr_all = OrderedDict((name, ([], [], [], [], [])) for name, _ in named)        # per clip: nmr wm / clean, audible wm / clean, cells
    classes = []
    for bi, s in enumerate(batches):
        s = s.to(device)
        message = (messages[bi].to(device) if messages is not None else
                   torch.randint(0, 2 ** message_bits, (s.shape[0],), device=device))
        if by_class:
            from .curate import clip_classes
            classes.append(clip_classes(s, SAMPLE_RATE))
        delta = postprocess(generator(s, message))
        both = torch.cat([s + delta, s], dim=0)
        for name, attack in named:
            attacked = both if attack is None else attack(both)
            out = _eval_reductions(detector(attacked), message, delta)
            for k, src in keys.items():
                acc[name][k].append(out[src])
            if "stoi" in quality:
                B = s.shape[0]
                d, kept = dsp.stoi(torch.cat([s, s], dim=0), attacked, SAMPLE_RATE)
                scored = (kept[:B] > 30) | torch.isnan(d[:B])                      # the mask is decided on s: one for both halves
                stoi_acc[name][0].append(d[:B][scored])
                stoi_acc[name][1].append(d[B:][scored])
                if by_class:
                    for dst, v in zip(stoi_all[name], (d[:B], d[B:], scored)):
                        dst.append(v)
            if "nmr" in quality:
                from .masking import masking
                B = s.shape[0]
                m = masking(torch.cat([s, s], dim=0), attacked, SAMPLE_RATE)
                for dst, v in zip(nmr_all[name], (m.nmr_db[:B], m.nmr_db[B:], m.audible[:B], m.audible[B:], m.cells[:B])):
                    dst.append(v)
    res = OrderedDict((name, {k: float(torch.cat(v).double().mean()) if v else math.nan for k, v in a.items()})
                      for name, a in acc.items())
    if "stoi" in quality:
        for name, (wm_half, clean_half) in stoi_acc.items():
            pooled = torch.cat(wm_half) if wm_half else torch.empty(0)
            res[name]["stoi"] = float(pooled.double().mean()) if pooled.numel() else math.nan
            res[name]["stoi_attack_only"] = float(torch.cat(clean_half).double().mean()) if pooled.numel() else math.nan
            res[name]["stoi_rows"] = int(pooled.numel())
    if "nmr" in quality:
        empty = (torch.empty(0), torch.empty(0), torch.empty(0, dtype=torch.int32), torch.empty(0, dtype=torch.int32),
                 torch.empty(0, dtype=torch.int32))
        nmr_cpu = {name: (tuple(torch.cat(v).cpu() for v in parts) if parts[0] else empty) for name, parts in nmr_all.items()}
        for name, parts in nmr_cpu.items():
            res[name].update(_nmr_pool(parts))
    if by_class:
        from .curate import CLASSES, class_report
        cls = torch.cat(classes) if classes else torch.empty(0, dtype=torch.int64)
        for name, a in acc.items():
            per = class_report({k: (torch.cat(v) if v else torch.empty(0)) for k, v in a.items()}, cls)
            if "stoi" in quality and stoi_all[name][0]:
                wm_half, clean_half, scored = (torch.cat(v).cpu() for v in stoi_all[name])
                for i, c in enumerate(CLASSES):
                    pick = (cls.cpu() == i) & scored
                    per[c]["stoi"] = float(wm_half[pick].double().mean()) if pick.any() else math.nan
                    per[c]["stoi_attack_only"] = float(clean_half[pick].double().mean()) if pick.any() else math.nan
                    per[c]["stoi_rows"] = int(pick.sum())
            elif "stoi" in quality:
                for c in CLASSES:
                    per[c].update(stoi=math.nan, stoi_attack_only=math.nan, stoi_rows=0)
            if "nmr" in quality:
                for i, c in enumerate(CLASSES):
                    per[c].update(_nmr_pool(nmr_cpu[name], (cls.cpu() == i) if nmr_cpu[name][0].numel() else None))
            res[name]["by_class"] = per
    return res
