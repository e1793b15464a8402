"""The 16-bit file codec as a step of the graph and of the save path.

main15c.ipynb (the reference's last notebook) trains and validates on what a saved file really holds: its
`perceptual_postprocess(x) = round(lowpass_biquad(x, 16000, 7000) * 32767) / 32767` is applied to s_w = s + delta in
train_one_epoch and validate_one_epoch.  py/main15.py:850-867 (save_audio) is the same filter followed by the truncating int16
cast.  On a CUDA tensor both are one launch of wm_biquad (ops.biquad) and the result stays on the device; a CPU tensor goes
through the host functions of inference.py, so that machines without a GPU can run them."""
from __future__ import annotations

import torch

from . import dsp

SAMPLE_RATE = 16000
GRAD_MODES = ("reference", "straight_through")


def _time_rows(x, name):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(x).__name__}")
    if x.dim() < 1 or x.dim() > 3 or x.numel() == 0:
        raise ValueError(f"{name}: expected (B, 1, T), (C, N) or (N,) with at least one sample, got shape {tuple(x.shape)}")
    return x


def perceptual_postprocess(x, cutoff=7000, sample_rate=SAMPLE_RATE, grad="reference"):
    """main15c's perceptual_postprocess: round(lowpass_biquad(x, sample_rate, cutoff) * 32767) / 32767 along the last axis of
    x ((B, 1, T), (C, N) or (N,)).  CUDA: one launch, the result stays on the device; grad="reference" makes it non-differentiable
    (torch.round's zero gradient), grad="straight_through" passes the gradient through rounding, clamp mask and the filter's adjoint
    (ops.PcmCodecFn).  CPU: the stated expression over inference.lowpass_biquad (grad="reference" only)."""
    if grad not in GRAD_MODES:
        raise ValueError(f"grad must be one of {GRAD_MODES}, got {grad!r}")
    coeffs = dsp.biquad_lowpass_coeffs(sample_rate, cutoff)
    x = _time_rows(x, "x")
    if x.is_cuda:
        return dsp.PcmCodecFn.apply(x.to(torch.float32), coeffs, grad)
    if grad != "reference":
        raise ValueError('grad="straight_through" needs a CUDA tensor: the CPU path has no adjoint filter')
    from .inference import lowpass_biquad
    return torch.round(lowpass_biquad(x, sample_rate, cutoff) * 32767) / 32767


class PcmCodec(torch.nn.Module):
    """perceptual_postprocess as a module: what forward_losses / train_step / eval_forward / evaluate_batches take as `codec=`"""

    def __init__(self, cutoff=7000, sample_rate=SAMPLE_RATE, grad="reference"):
        super().__init__()
        if grad not in GRAD_MODES:
            raise ValueError(f"grad must be one of {GRAD_MODES}, got {grad!r}")
        dsp.biquad_lowpass_coeffs(sample_rate, cutoff)              # bad rates fail here
        self.cutoff, self.sample_rate, self.grad = cutoff, sample_rate, grad

    def forward(self, x):
        return perceptual_postprocess(x, self.cutoff, self.sample_rate, self.grad)

    def extra_repr(self):
        return f"cutoff={self.cutoff}, sample_rate={self.sample_rate}, grad={self.grad!r}"


def encode_pcm16(waveform, sample_rate=SAMPLE_RATE, lowpass_hz=7000):
    """The samples save_audio writes (py/main15.py:850-867), as an int16 (C, N) tensor on the waveform's device: biquad low-pass at
    `lowpass_hz` -> clamp -> x32767 -> truncating int16 cast.  lowpass_hz=None: the quantiser alone.  CUDA: one launch;
    CPU: pcm16(lowpass_biquad(waveform))."""
    x = _time_rows(waveform, "waveform").detach()
    if x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dim() != 2:
        raise ValueError(f"waveform: expected (channels, samples) or (samples,), got shape {tuple(waveform.shape)}")
    coeffs = dsp.BIQUAD_IDENTITY if lowpass_hz is None else dsp.biquad_lowpass_coeffs(sample_rate, lowpass_hz)
    if x.is_cuda:
        return dsp.biquad(x.to(torch.float32), coeffs, mode="pcm16")
    from .inference import lowpass_biquad, pcm16
    return pcm16(x if lowpass_hz is None else lowpass_biquad(x, sample_rate, cutoff_freq=lowpass_hz))
