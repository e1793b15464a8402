"""File-level embed / detect: the reference chops a recording into 1-s segments and calls the
models at B=1 per segment in a Python loop (py/main16.py:977-1066, :1114-1207, :723-762).  Here ALL segments of a
recording go through the HIP path as one [N,1,16000] batch; per-segment random messages, remainder pad/trim and the
returned dict schemas are the reference's.  Like the reference's wrappers (and unlike its training loop) no
fir/clamp/rms post-processing is applied to delta.  A recording that is not at 16 kHz is mixed down,
resampled and cut into those segments by one launch (`orig_freq=`, ops.resample; `resample` / `Resample` / `load_audio` here)."""
from __future__ import annotations

import math
import os
import wave

import numpy as np
import torch
import torch.nn.functional as F

SAMPLE_RATE = 16000


def _as_channels(waveform):
    """(N,) or (C, N) -> (C, N) float32"""
    if not isinstance(waveform, torch.Tensor):
        raise TypeError(f"waveform: expected a tensor, got {type(waveform).__name__}")
    x = waveform.unsqueeze(0) if waveform.dim() == 1 else waveform
    if x.dim() != 2:
        raise ValueError(f"waveform: expected (channels, samples) or (samples,), got shape {tuple(waveform.shape)}")
    return x.to(torch.float32)


def _resample_rows_host(x, orig_freq, new_freq, length=None):
    """CPU twin of ops.resample_rows: every row of the float32 (rows, N) tensor by itself through the float32 `dense` table as one strided
    F.conv1d per row (a row's samples do not depend on its neighbours or on their number); the first `length` samples of each, all
    ceil(new * N / orig) by default.  Plain torch operations: autograd differentiates it."""
    from . import dsp
    tab = dsp.resample_table(orig_freq, new_freq)
    P, width = tab["P"], tab["width"]
    n = dsp.resample_length(x.shape[1], orig_freq, new_freq) if length is None else length
    padded = F.pad(x, (width, width + P))
    weight = tab["dense"][:, None, :]
    # (1, Q, N // P + 1): [phase][period] per row
    return torch.stack([F.conv1d(row[None, None], weight, stride=P).transpose(1, 2).reshape(-1)[:n] for row in padded]).contiguous()


def resample(waveform, orig_freq, new_freq, mixdown=True):
    """torchaudio.functional.resample(waveform, orig_freq, new_freq) with its documented defaults (sinc_interp_hann,
    lowpass_filter_width=6, rolloff=0.99), restated from the published description (ops.resample_table), preceded by the mono
    mixdown every file-level entry point of the reference applies first (py/main16.py:717-720): a (C, N) or (N,) waveform
    becomes (1, ceil(new * N / orig)).  A CUDA tensor goes to the HIP kernel (ops.resample); a CPU tensor goes through the same
    float32 table as one strided F.conv1d -- the only CPU arithmetic here, it is what lets load_audio read a 48 kHz file on a
    machine without a GPU.  Equal rates return the waveform unchanged.
    mixdown=False filters every channel by itself, as torchaudio.functional.resample does: (C, N) -> (C, L), (N,) -> (1, L)
    (ops.resample_rows on CUDA, the same conv1d per channel on the CPU).
    PARITY WITH TORCHAUDIO UNPINNED: torchaudio is absent from this image; tests/test_resample_cpu.py pins it on the first
    machine that has it."""
    from . import dsp
    tab = dsp.resample_table(orig_freq, new_freq)
    if tab["K"] == 1:
        return waveform
    x = _as_channels(waveform)
    if not mixdown:
        return dsp.resample_rows(x, orig_freq, new_freq) if x.is_cuda else _resample_rows_host(x, orig_freq, new_freq)
    if x.is_cuda:
        return dsp.resample(x, orig_freq, new_freq)
    # channels added in float64, one rounding to float32 (as the kernel does): the mean's error is an ulp of the mean, also where channels cancel
    mono = x.double().mean(dim=0, keepdim=True).float() if x.shape[0] > 1 else x
    P, Q, width = tab["P"], tab["Q"], tab["width"]
    n = mono.shape[1]
    padded = F.pad(mono, (width, width + P))
    y = F.conv1d(padded[None], tab["dense"][:, None, :], stride=P)                 # (1, Q, n // P + 1): [phase][period]
    return y.transpose(1, 2).reshape(1, -1)[:, :dsp.resample_length(n, orig_freq, new_freq)].contiguous()


class Resample(torch.nn.Module):
    """torchaudio.transforms.Resample(orig_freq, new_freq) for code written against it: calls `resample`"""

    def __init__(self, orig_freq=SAMPLE_RATE, new_freq=SAMPLE_RATE):
        super().__init__()
        from . import dsp
        dsp.resample_table(orig_freq, new_freq)          # bad rates fail here, as torchaudio's constructor does
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)

    def forward(self, waveform):
        return resample(waveform, self.orig_freq, self.new_freq)


def resample_add(x, delta, orig_freq, delta_freq=SAMPLE_RATE):
    """The way back of `resample`: `delta` (at delta_freq, read flat) taken to the rate `orig_freq` of the recording `x` ((C, N) or (N,))
    and added to every channel of it.  Of delta the first n_d = ceil(delta_freq * N / orig_freq) samples count (fewer: ValueError); what
    lies behind them is ignored.  Returns (out (C, N), up (1, N)): up is resample(delta[:n_d], delta_freq, orig_freq)[:, :N] and
    out[c] = x[c] + up[0].  CUDA tensors go to the HIP kernel (ops.resample_add, one launch); CPU tensors through the CPU twin of
    `resample` and one add."""
    from . import dsp
    dsp.resample_table(delta_freq, orig_freq)                        # bad rates fail here
    x = _as_channels(x)
    if not isinstance(delta, torch.Tensor):
        raise TypeError(f"delta: expected a tensor, got {type(delta).__name__}")
    n = x.shape[1]
    n_d = dsp.resample_length(n, orig_freq, delta_freq)
    if delta.numel() < n_d:
        raise ValueError(f"delta: {n} samples at {orig_freq} Hz need {n_d} at {delta_freq} Hz, got {delta.numel()}")
    if x.is_cuda:
        return dsp.resample_add(x.contiguous(), delta.to(torch.float32).contiguous(), orig_freq, delta_freq)
    d = delta.to(torch.float32).reshape(1, -1)[:, :n_d]
    up = resample(d, delta_freq, orig_freq)[:, :n]
    up = up.clone() if up.data_ptr() == delta.data_ptr() else up.contiguous()     # equal rates hand delta itself back: never a view of it
    return x + up, up


def read_audio(file_path):
    """((C, N) float32 waveform, sample rate): the file's own channels at the file's own rate -- what `native_rate=True` embeds into.
    torchaudio.load where it is installed, else the .wav reader of load_audio."""
    try:
        import torchaudio
    except ImportError:
        data, rate = _read_wav(file_path)
        return torch.from_numpy(np.ascontiguousarray(data.T)), int(rate)
    waveform, sr = torchaudio.load(file_path)
    return waveform.to(torch.float32), int(sr)


def load_audio(file_path, sample_rate=SAMPLE_RATE, device=None):
    """(1, N) fp32 mono waveform at `sample_rate`.  Uses torchaudio when it is installed (the reference's loader, :714-720).
    Otherwise .wav files (16- / 24-bit PCM, 32-bit float, plain or WAVE_FORMAT_EXTENSIBLE header) are read with the standard
    library, mixed down to mono and, when the file is at another rate, resampled with `resample`.  `device` (e.g. "cuda"):
    the decoded (C, N) samples are uploaded once and mixdown + resampling run on the GPU; the result stays there."""
    try:
        import torchaudio  # noqa: F401
        waveform, sr = torchaudio.load(file_path)
        if waveform.shape[0] > 1:
            waveform = waveform.mean(dim=0, keepdim=True)
        if sr != sample_rate:
            waveform = torchaudio.transforms.Resample(sr, sample_rate)(waveform)
        return waveform if device is None else waveform.to(device)
    except ImportError:
        data, rate = _read_wav(file_path)
        if device is not None and torch.device(device).type != "cpu":
            x = torch.from_numpy(np.ascontiguousarray(data.T)).to(device)
            if rate != sample_rate:
                return resample(x, rate, sample_rate)
            return x.mean(dim=0, keepdim=True) if x.shape[0] > 1 else x
        if rate != sample_rate:
            return resample(torch.from_numpy(np.ascontiguousarray(data.T)), rate, sample_rate)
        return torch.from_numpy(data.mean(axis=1).astype(np.float32)).unsqueeze(0)


def _read_wav(path):
    """RIFF/WAVE reader: 16-bit and 24-bit signed PCM (format 1, scaled by 1/32768 and 1/2**23 as torchaudio.load normalises
    them) and 32-bit IEEE float (format 3), under a plain header or WAVE_FORMAT_EXTENSIBLE (format 0xFFFE, where the first two
    bytes of the sub-format GUID carry the code).  Returns ((frames, channels) float32, sample rate)."""
    import struct
    with open(path, "rb") as f:
        blob = f.read()
    if blob[:4] != b"RIFF" or blob[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, data, ext = 12, None, None, None
    while pos + 8 <= len(blob):
        tag, size = blob[pos:pos + 4], struct.unpack("<I", blob[pos + 4:pos + 8])[0]
        body = blob[pos + 8:pos + 8 + size]
        if tag == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
            ext = struct.unpack("<H", body[24:26])[0] if len(body) >= 40 else None
        elif tag == b"data":
            data = body
        pos += 8 + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError(f"{path}: missing fmt or data chunk")
    code, channels, rate, _, _, bits = fmt
    if code == 0xFFFE:
        if ext is None:
            raise ValueError(f"{path}: WAVE_FORMAT_EXTENSIBLE header without a sub-format")
        code = ext
    if code == 1 and bits == 16:
        x = np.frombuffer(data, dtype="<i2").astype(np.float32) / 32768.0
    elif code == 1 and bits == 24:
        b = np.frombuffer(data[:len(data) - len(data) % 3], dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = (v - ((v & 0x800000) << 1)).astype(np.float32) / 8388608.0
    elif code == 3 and bits == 32:
        x = np.frombuffer(data, dtype="<f4").astype(np.float32)
    else:
        raise ValueError("without torchaudio only 16- / 24-bit PCM and 32-bit float wav files can be read")
    return x.reshape(-1, channels), rate


def save_audio_float(waveform, output_path, sample_rate=SAMPLE_RATE):
    """py/main16.py:802-804 / :1051-1055: `torchaudio.save(path, float_waveform, sample_rate)` stores a float tensor as a
    32-bit IEEE-float WAV (samples bit for bit).  Written here as a plain RIFF file (format tag 3)."""
    import struct
    out_dir = os.path.dirname(output_path)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    x = waveform.detach().cpu().to(torch.float32)
    if x.dim() == 1:
        x = x.unsqueeze(0)
    ch = x.shape[0]
    payload = np.ascontiguousarray(x.numpy().T).astype("<f4").tobytes()
    hdr = (b"RIFF" + struct.pack("<I", 36 + len(payload)) + b"WAVE" + b"fmt " +
           struct.pack("<IHHIIHH", 16, 3, ch, sample_rate, sample_rate * ch * 4, ch * 4, 32) + b"data" + struct.pack("<I", len(payload)))
    with open(output_path, "wb") as f:
        f.write(hdr + payload)


def lowpass_biquad(waveform, sample_rate, cutoff_freq, Q=0.707):
    """torchaudio.functional.lowpass_biquad (imported at py/main15.py:18, called at :855), restated from its published
    definition: the RBJ cookbook low-pass section  b = ((1-cos w0)/2, 1-cos w0, (1-cos w0)/2),  a = (1+alpha, -2 cos w0, 1-alpha)
    with w0 = 2 pi cutoff / sample_rate and alpha = sin w0 / (2 Q), normalised by a0, run along the last axis as an IIR filter
    in the waveform's dtype, and the output clamped to [-1, 1] (torchaudio's `lfilter(..., clamp=True)` default).
    PARITY UNPINNED: torchaudio is absent from this image and the reference holds no fixture of this function; the order of
    the fp32 additions inside torchaudio's lfilter (direct form I) is not reproduced bit for bit -- scipy's lfilter
    (transposed direct form II) carries the recursion here."""
    from scipy.signal import lfilter
    w0 = 2.0 * math.pi * float(cutoff_freq) / float(sample_rate)
    alpha = math.sin(w0) / (2.0 * float(Q))
    cw = math.cos(w0)
    b = np.array([(1.0 - cw) / 2.0, 1.0 - cw, (1.0 - cw) / 2.0], dtype=np.float64)
    a = np.array([1.0 + alpha, -2.0 * cw, 1.0 - alpha], dtype=np.float64)
    x = waveform.detach().cpu()
    y = lfilter((b / a[0]).astype(np.float32), (a / a[0]).astype(np.float32), x.to(torch.float32).numpy(), axis=-1)
    return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).clamp_(-1.0, 1.0).to(x.dtype)


def pcm16(waveform):
    """float waveform -> signed 16-bit PCM exactly as py/main15.py:858: clamp to [-1, 1], scale by 32767, and the
    TRUNCATING float -> int16 conversion of `.to(torch.int16)` (toward zero; no rounding)."""
    return (waveform.detach().cpu().clamp(-1.0, 1.0) * 32767).to(torch.int16)


def save_audio(waveform, output_path, sample_rate=SAMPLE_RATE, lowpass_hz=7000, device=None):
    """py/main15.py:850-867 `save_audio(waveform, output_path, sample_rate)`: 7 kHz biquad low-pass -> clamp -> x32767 ->
    truncating int16 cast -> 16-bit signed PCM WAV.  The container is written with the standard library (`torchaudio.save(...,
    encoding="PCM_S", bits_per_sample=16)` in the reference; a mono or (C, N) waveform, samples interleaved by channel).
    `lowpass_hz=None` skips the filter (the PCM bytes are then exactly pcm16(waveform)).
    `device` (e.g. "cuda"): filter and quantiser run there as one launch (codec.encode_pcm16; the waveform is uploaded if it is not
    there yet) and int16 codes come back, half the bytes of the float waveform.  None: the host path, also for a CUDA waveform."""
    out_dir = os.path.dirname(output_path)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    if device is not None and torch.device(device).type != "cpu":
        from .codec import encode_pcm16
        pcm = encode_pcm16(waveform.detach().to(device), sample_rate, lowpass_hz).cpu().numpy()
    else:
        x = waveform.detach().cpu()
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if lowpass_hz is not None:
            x = lowpass_biquad(x, sample_rate, cutoff_freq=lowpass_hz)
        pcm = pcm16(x).numpy()                               # (C, N)
    with wave.open(output_path, "wb") as w:
        w.setnchannels(pcm.shape[0]); w.setsampwidth(2); w.setframerate(sample_rate)
        w.writeframes(np.ascontiguousarray(pcm.T).astype("<i2").tobytes())


def _segments(waveform, seg_len=SAMPLE_RATE):
    """(1,N) -> ([S,1,seg_len] batch with a zero-padded last segment, remainder length)"""
    total = waveform.shape[1]
    num_full, remainder = total // seg_len, total % seg_len
    segs = [waveform[:, i * seg_len:(i + 1) * seg_len] for i in range(num_full)]
    if remainder > 0:
        segs.append(F.pad(waveform[:, num_full * seg_len:], (0, seg_len - remainder)))
    if not segs:
        return waveform.new_zeros(0, 1, seg_len), 0
    return torch.stack(segs, dim=0), remainder


def _ingest(waveform, orig_freq, device, seg_len=SAMPLE_RATE):
    """(segments [S,1,seg_len], remainder, the (1, n) waveform at the model rate) for a wrapper's `waveform` argument.
    orig_freq None (or already the model rate): the (1, N) waveform is cut on the host, as before.  Any other rate: the
    (C, N) waveform at that rate is uploaded once and ops.resample does mixdown, resampling, tail padding and segment
    stacking in one launch; the segments stay on the device and the 16 kHz waveform is a view of them."""
    if orig_freq is None or int(orig_freq) == seg_len:
        segs, remainder = _segments(waveform.float(), seg_len)
        return segs, remainder, waveform
    from . import dsp
    x = _as_channels(waveform).to(device)
    segs = dsp.resample(x, orig_freq, seg_len, seg_len=seg_len)
    n = dsp.resample_length(x.shape[1], orig_freq, seg_len)
    return segs, n % seg_len, segs.reshape(1, -1)[:, :n]


def _si_snr_db(ref, est, eps):
    """scale-invariant SNR in dB along axis 1: both signals centred, `est` split into its projection on `ref` and the rest,
    10 log10 of the energy ratio (eps added to the projection's denominator and to the residual energy, as py/main16.py:764-773)"""
    ref = ref - ref.mean(dim=1, keepdim=True)
    est = est - est.mean(dim=1, keepdim=True)
    gain = (ref * est).sum(dim=1, keepdim=True) / (ref.pow(2).sum(dim=1, keepdim=True) + eps)
    proj = gain * ref
    resid = est - proj
    return 10 * torch.log10(proj.pow(2).sum(dim=1) / (resid.pow(2).sum(dim=1) + eps))


def compute_si_snr(s, s_hat, eps=1e-8):
    """py/main16.py:764-773: mean SI-SNR (dB) of `s_hat` against `s`, as a Python float"""
    return _si_snr_db(s, s_hat, eps).mean().item()


@torch.no_grad()
def embed_waveform(waveform, generator, message_bits=16, device="cuda", messages=None, max_batch=512, orig_freq=None, native_rate=False):
    """process_audio_file_with_delta (:723-762) on an in-memory waveform, batched.
    Returns (watermarked_waveform, delta_waveform, original_waveform), each (1, N) on the CPU.  `orig_freq`: the rate of a
    (C, N) waveform that is not at 16 kHz yet (see _ingest); the three returned waveforms are at 16 kHz, as the reference's.
    `native_rate=True` (no counterpart in the reference): the recording keeps its channels and its rate.  The (C, N) waveform at
    `orig_freq` (None: 16 kHz) is uploaded once, its mixdown at 16 kHz feeds the generator as above, the batches write delta into one
    (S, 1, 16000) device buffer and ONE wm_resample_add launch takes that delta up to `orig_freq` and adds it to every channel of the
    untouched recording.  Returns (watermarked (C, N), delta (1, N), original (C, N)) on the CPU at `orig_freq`."""
    generator.eval()
    if native_rate:
        return _embed_native(waveform, generator, message_bits, device, messages, max_batch, orig_freq)
    segs, remainder, waveform = _ingest(waveform, orig_freq, device)
    S = segs.shape[0]
    if S == 0:
        waveform = waveform.cpu()
        return waveform.clone(), torch.zeros_like(waveform), waveform
    if messages is None:       # a fresh random message per second, as :1001
        messages = torch.randint(0, 2 ** message_bits, (S,), device=device)
    deltas = []
    for i in range(0, S, max_batch):
        x = segs[i:i + max_batch].to(device)
        deltas.append(generator(x, messages[i:i + max_batch].to(device)).cpu())
    delta = torch.cat(deltas, dim=0)                    # [S,1,16000]
    wm = segs.cpu() + delta
    n = waveform.shape[1]
    delta_w = delta.reshape(1, -1)[:, :n]
    wm_w = wm.reshape(1, -1)[:, :n]
    return wm_w, delta_w, waveform.cpu()


def _embed_native(waveform, generator, message_bits, device, messages, max_batch, orig_freq, seg_len=SAMPLE_RATE):
    """embed_waveform(native_rate=True): everything between the upload of the recording and the download of the result stays on the device.
    The segments come from the launch _ingest uses for a recording that is not at 16 kHz, called here directly: _ingest cuts a 16 kHz
    waveform on the host without a mixdown (the old call, which must not change) and does not hand back the uploaded (C, N) channels that
    wm_resample_add adds delta to."""
    from . import dsp
    rate = seg_len if orig_freq is None else dsp._rate(orig_freq, "orig_freq")
    original = _as_channels(waveform)
    x = original.to(device).contiguous()
    segs = dsp.resample(x, rate, seg_len, seg_len=seg_len)           # (S, 1, seg_len): mixdown (+ resampling) + tail padding, one launch
    S = segs.shape[0]
    if S == 0:
        original = original.cpu()
        return original.clone(), original.new_zeros(1, 0), original
    if messages is None:       # a fresh random message per second, as :1001
        messages = torch.randint(0, 2 ** message_bits, (S,), device=device)
    delta = torch.empty_like(segs)
    for i in range(0, S, max_batch):
        delta[i:i + max_batch] = generator(segs[i:i + max_batch], messages[i:i + max_batch].to(device))
    wm, up = dsp.resample_add(x, delta, rate, seg_len)               # Nd = n16: the generator's output for the zero tail is not read
    return wm.cpu(), up.cpu(), original.cpu()


def generate_watermarked_audio(input_file, generator, output_file=None, message_bits=16, device="cuda", orig_freq=None, native_rate=False,
                               stoi=False, nmr=False):
    """py/main16.py:977-1066 with one batched Generator call; same result dict.  A path is loaded (and resampled) by
    load_audio; `orig_freq` is the rate of an in-memory (C, N) waveform that is not at 16 kHz.
    `native_rate=True`: a path is read by read_audio (its channels, its rate), an in-memory (C, N) waveform is at `orig_freq`; the three
    waveforms come back at that rate with all channels (embed_waveform), `output_file` is written at that rate with all channels, the
    metrics are taken at that rate (SI-SNR over the channel rows) and the dict gains "sample_rate".
    `stoi=True` adds metrics["stoi"]: STOI (quality.stoi) of the watermarked against the original waveform, the whole recording as ONE
    row per channel at the rate the waveforms come back at, averaged over the channels; one upload, one wm_stoi call.
    `nmr=True` adds metrics["nmr_db"] and metrics["audible_share"] (masking.masking: one simultaneous-masking model at an assumed playback
    level) of the watermarked against the original waveform, the whole recording as ONE row per channel: the noise-to-mask ratio in dB
    averaged over the channels, and audible cells / cells over all of them; one wm_masking_fwd call."""
    if native_rate:
        if isinstance(input_file, (str, os.PathLike)):
            waveform, rate = read_audio(input_file)
        else:
            waveform, rate = input_file, (SAMPLE_RATE if orig_freq is None else int(orig_freq))
        wm, delta, orig = embed_waveform(waveform, generator, message_bits=message_bits, device=device, orig_freq=rate, native_rate=True)
    else:
        if isinstance(input_file, (str, os.PathLike)):
            waveform, orig_freq = load_audio(input_file), None
        else:
            waveform = input_file
        wm, delta, orig = embed_waveform(waveform, generator, message_bits=message_bits, device=device, orig_freq=orig_freq)
        rate = SAMPLE_RATE
    watermark_rms = torch.sqrt((delta ** 2).mean()).item()
    si_snr = compute_si_snr(orig, wm)
    power_ratio_db = 10 * np.log10(torch.mean(orig ** 2).item() / max(torch.mean(delta ** 2).item(), 1e-30))
    if output_file:
        save_audio_float(wm, output_file, rate)           # :1051-1055 stores the float waveform as is
    result = {"watermarked_waveform": wm, "delta_waveform": delta, "original_waveform": orig,
              "metrics": {"watermark_rms": watermark_rms, "si_snr_db": si_snr, "power_ratio_db": power_ratio_db}}
    if stoi:
        result["metrics"]["stoi"] = _stoi_whole(orig, wm, rate, device)
    if nmr:
        result["metrics"]["nmr_db"], result["metrics"]["audible_share"] = _nmr_whole(orig, wm, rate, device)
    if native_rate:
        result["sample_rate"] = rate
    return result


def _stoi_whole(original, processed, rate, device):
    """STOI of a whole (C, N) recording against its original, every channel as one row (the long-row path of wm_stoi), mean over channels"""
    from . import dsp
    d, _ = dsp.stoi(_as_channels(original).to(device), _as_channels(processed).to(device), rate)
    return float(d.double().mean())


def _nmr_whole(original, processed, rate, device):
    """(nmr_db averaged over the channels, audible cells / cells) of a whole (C, N) recording against its original, every channel as one row"""
    from .masking import masking
    m = masking(_as_channels(original).to(device), _as_channels(processed).to(device), rate)
    cells = int(m.cells.sum())
    return float(m.nmr_db.double().mean()), (int(m.audible.sum()) / cells if cells else math.nan)


@torch.no_grad()
def detect_waveform(waveform, detector, detection_threshold=0.5, device="cuda", max_batch=512, orig_freq=None):
    """detect_watermark (:1114-1207) on an in-memory waveform, batched; same result dict (no plotting).  The
    per-segment reductions run on the device: only the temporal probability track the reference returns ((N,) floats)
    and 1+bits scalars cross to the host, never the [S,T,1+bits] logits.  `orig_freq`: the rate of a (C, N) waveform that is
    not at 16 kHz yet (see _ingest); the temporal track is then at 16 kHz."""
    detector.eval()
    segs, remainder, waveform = _ingest(waveform, orig_freq, device)
    S = segs.shape[0]
    n = waveform.shape[1]
    bits = int(getattr(detector, "message_bits", 0))
    probs, seg_logit_means = [], []
    for i in range(0, S, max_batch):
        logits = detector(segs[i:i + max_batch].to(device))            # [s,T,1+bits]
        probs.append(torch.sigmoid(logits[:, :, 0]))
        if bits > 0:
            ml = logits[:, :, 1:]
            last = (i + ml.shape[0] == S) and remainder > 0
            m = ml.mean(dim=1)                                          # per-segment mean over its samples (:1142)
            if last:                                                    # the remainder segment: valid samples only (:1162)
                m = torch.cat([m[:-1], ml[-1, :remainder].mean(dim=0, keepdim=True)], dim=0)
            seg_logit_means.append(m)
    temporal = torch.cat(probs, dim=0).reshape(-1)[:n]                  # [N] on the device
    mean_prob = temporal.mean().item()
    is_wm = mean_prob > detection_threshold
    result = {"mean_probability": mean_prob, "is_watermarked": is_wm, "temporal_probs": temporal.cpu().numpy(),
              "decision": "WATERMARKED" if is_wm else "NOT WATERMARKED"}
    if seg_logit_means:
        mean_logits = torch.cat(seg_logit_means, dim=0).mean(dim=0)
        result["predicted_message"] = (mean_logits > 0).int().tolist()
        result["message_confidence"] = torch.sigmoid(mean_logits).tolist()
    return result


def detect_watermark(input_file, detector, detection_threshold=0.5, visualize=False, device="cuda", orig_freq=None):
    if isinstance(input_file, (str, os.PathLike)):
        waveform, orig_freq = load_audio(input_file), None
    else:
        waveform = input_file
    return detect_waveform(waveform, detector, detection_threshold, device, orig_freq=orig_freq)


def merge_short_runs(bits, min_len):
    """Runs of equal values of the bool array `bits` as a list of [start, end, value] (end exclusive), after runs shorter than `min_len`
    samples were merged into their neighbours: while there is more than one run and the shortest is shorter than min_len, the FIRST of
    the shortest runs takes its neighbours' value (they agree: runs alternate) and the three, or two at an end, become one run."""
    bits = np.asarray(bits, dtype=bool).reshape(-1)
    if bits.size == 0:
        return []
    edges = np.flatnonzero(bits[1:] != bits[:-1]) + 1
    starts, ends = np.concatenate([[0], edges]), np.concatenate([edges, [bits.size]])
    runs = [[int(a), int(b), bool(bits[a])] for a, b in zip(starts, ends)]
    while len(runs) > 1:
        lens = [b - a for a, b, _ in runs]
        i = int(np.argmin(lens))                                        # the first of the shortest
        if lens[i] >= min_len:
            break
        lo, hi = max(i - 1, 0), min(i + 1, len(runs) - 1)
        runs[lo:hi + 1] = [[runs[lo][0], runs[hi][1], not runs[i][2]]]
    return runs


@torch.no_grad()
def locate_watermark(waveform_or_path, detector, threshold=0.5, min_len_s=0.02, device="cuda", max_batch=512, orig_freq=None):
    """WHERE a recording is watermarked: the Detector's per-sample track, thresholded on the device, as intervals in seconds.
    Returns {"watermarked": [(start_s, end_s), ...], "unmarked": the same, "fraction_watermarked"}: the two lists tile the recording;
    the fraction is the share of samples whose own prediction is 1, before any merging (NaN for an empty recording).
    The prediction sigmoid(logits[:, :, 0]) > threshold leaves the device as the packed bit mask of ops.loc_counts -- n / 8 bytes, not
    the 4n-byte probability track detect_waveform returns -- and runs shorter than min_len_s are merged into their neighbours on the host
    (merge_short_runs).  A path is read by load_audio; `orig_freq` is the rate of an in-memory (C, N) waveform that is not at 16 kHz
    (see _ingest; the intervals are then in seconds all the same).  The shipped checkpoints were never trained to localise: what
    this returns for a spliced recording is whatever attacks.evaluate_localization measures, not a promise."""
    from . import dsp
    from .attacks import unpack_labels
    if isinstance(min_len_s, bool) or not isinstance(min_len_s, (int, float)) or not math.isfinite(min_len_s) or min_len_s < 0:
        raise ValueError(f"min_len_s: expected a non-negative number of seconds, got {min_len_s!r}")
    dsp.loc_threshold_logit(threshold)                                  # a bad threshold fails here
    if isinstance(waveform_or_path, (str, os.PathLike)):
        waveform, orig_freq = load_audio(waveform_or_path), None
    else:
        waveform = waveform_or_path
    detector.eval()
    segs, _, waveform = _ingest(waveform, orig_freq, device)
    S, n, T = segs.shape[0], waveform.shape[1], segs.shape[2]
    if S == 0 or n == 0:
        return {"watermarked": [], "unmarked": [], "fraction_watermarked": math.nan}
    masks = []
    for i in range(0, S, max_batch):
        logits = detector(segs[i:i + max_batch].to(device))            # [s,T,1+bits]: stays on the device
        masks.append(dsp.loc_counts(logits, None, threshold, want_pred=True)[1])
    pred = unpack_labels(torch.cat(masks, dim=0), T).reshape(-1)[:n]
    out = {"watermarked": [], "unmarked": [], "fraction_watermarked": float(pred.mean())}
    for a, b, v in merge_short_runs(pred, min_len_s * SAMPLE_RATE):
        out["watermarked" if v else "unmarked"].append((a / SAMPLE_RATE, b / SAMPLE_RATE))
    return out


@torch.no_grad()
def detect_prob(file_path, detector, sample_rate=SAMPLE_RATE, device="cuda", max_batch=512, orig_freq=None):
    """py/main16.py:1575-1596: average over the file's 1-s segments of each segment's mean detection probability.  The
    mean of a segment runs over all 16 000 samples of the zero-PADDED tail segment too (unlike detect_watermark, which
    trims it), so this is a mean of per-segment means, not the mean of the temporal track.  One batched Detector call;
    accepts a path or an in-memory (1,N) waveform, or a (C,N) one at `orig_freq` (see _ingest)."""
    if isinstance(file_path, (str, os.PathLike)):
        waveform, orig_freq = load_audio(file_path, sample_rate), None
    else:
        waveform = file_path
    segs, _, _ = _ingest(waveform, orig_freq, device, sample_rate)
    if segs.shape[0] == 0:
        return float("nan")                                             # np.mean([]) in the reference
    seg_means = []
    for i in range(0, segs.shape[0], max_batch):
        logits = detector(segs[i:i + max_batch].to(device))
        seg_means.append(torch.sigmoid(logits[:, :, 0]).mean(dim=1))
    return float(torch.cat(seg_means).double().mean().item())


def _si_snr_rows(s, s_hat, eps=1e-8):
    """compute_si_snr (:764-773) applied to each (1,1,T) segment of a [S,1,T] batch, as evaluate_unseen_file does
    (:1294): the reductions run over dim=1 -- for a 3-D segment that is the size-1 CHANNEL axis, so s - mean == 0 and
    every segment yields 10*log10(0/eps) = -inf.  Kept as is (reference quirk; call compute_si_snr on (1,N) waveforms
    for a meaningful value).  Returns [S] per-segment values."""
    return _si_snr_db(s, s_hat, eps).mean(dim=1)


@torch.no_grad()
def evaluate_unseen_file(filepath, generator, detector, device="cuda", message_bits=16, messages=None, max_batch=256,
                         orig_freq=None, stoi=False, nmr=False):
    """py/main16.py:1263-1299 with all 1-s segments of the file as one batch: returns (mean clean detection probability,
    mean watermarked detection probability, mean SI-SNR, mean delta RMS) over the segments, or four Nones when the file
    cannot be read (:1264-1267).  A fresh random message per segment (:1287) unless `messages` is given.  Accepts a path
    or an in-memory (1,N) waveform, or a (C,N) one at `orig_freq` (see _ingest).  Per-segment reductions run on the device;
    four scalars come back.
    `stoi=True`: a fifth element, STOI (quality.stoi) of the whole 16 kHz recording as ONE row, watermarked against original (the
    reference's baseline variant averages pystoi over the one-second segments instead, py/main14.py:1099-1203); five Nones when the
    file cannot be read.
    `nmr=True`: one more element behind that, the noise-to-mask ratio in dB (masking.masking) of the whole 16 kHz recording as ONE row,
    watermarked against original."""
    nout = 4 + bool(stoi) + bool(nmr)
    if isinstance(filepath, (str, os.PathLike)):
        try:
            waveform, orig_freq = load_audio(filepath), None
        except Exception:
            return (None,) * nout
    else:
        waveform = filepath
    generator.eval(); detector.eval()
    segs, remainder, _ = _ingest(waveform, orig_freq, device)
    S = segs.shape[0]
    if S == 0:
        return (float("nan"),) * nout
    if messages is None:
        messages = torch.randint(0, 2 ** message_bits, (S,), device=device)
    clean, wm, si, rms = [], [], [], []
    whole = torch.empty(S, 1, segs.shape[2], device=device) if stoi or nmr else None   # the watermarked segments, for the one-row measures
    for i in range(0, S, max_batch):
        seg = segs[i:i + max_batch].to(device)
        delta = generator(seg, messages[i:i + max_batch].to(device))
        seg_w = seg + delta
        p = torch.sigmoid(detector(torch.cat([seg, seg_w], dim=0))[:, :, 0]).mean(dim=1)    # eval-mode BN: rows independent
        k = seg.shape[0]
        clean.append(p[:k]); wm.append(p[k:])
        rms.append(torch.sqrt((delta ** 2).mean(dim=[1, 2])))
        si.append(_si_snr_rows(seg, seg_w))
        if whole is not None:
            whole[i:i + k] = seg_w
    out = torch.stack([torch.cat(v).double().mean() for v in (clean, wm, si, rms)]).cpu()
    res = tuple(float(v) for v in out)
    if whole is not None:
        n = (S - 1) * segs.shape[2] + (remainder if remainder else segs.shape[2])     # the recording without the last segment's padding
    if stoi:
        from . import dsp
        d, _ = dsp.stoi(segs.to(device).reshape(1, -1)[:, :n], whole.reshape(1, -1)[:, :n], SAMPLE_RATE)
        res += (float(d[0]),)
    if nmr:
        from .masking import masking
        m = masking(segs.to(device).reshape(1, -1)[:, :n].contiguous(), whole.reshape(1, -1)[:, :n].contiguous(), SAMPLE_RATE)
        res += (float(m.nmr_db[0]),)
    return res


@torch.no_grad()
def evaluate_batches(generator, detector, batches, device="cuda", message_bits=16, threshold=0.5, messages=None, codec=None, tamper=None,
                     by_class=False):
    """evaluate_model (:369-423): the per-batch reductions run on the device (step.eval_forward); the per-clip values of
    all batches are pooled and averaged once, as the reference's np.mean over its extended lists does (so a ragged last
    batch weighs by its clips).  `messages` (optional list, one tensor per batch) replaces the randint draw of :381.
    `codec` (a codec.PcmCodec): the Detector is evaluated on codec(s + delta), as in main15c's validate_one_epoch.
    `tamper` (an attacks.Splice): the watermarked half is spliced behind the codec (step.eval_forward); the averages are the same ones, so
    the watermarked probability falls with the share that was cut out -- attacks.evaluate_localization scores the per-sample track.
    `by_class=True` adds "by_class": {"speech" | "noise" | "silent": {"clips": count, and the four keys over that class's clips (NaN for
    an empty class)}}, the classes being curate.clip_classes of the clean batch (one wm_clip_features launch per batch; a clip with a
    non-finite sample is in none).  The default returns the dict as it was."""
    from .step import eval_forward
    generator.eval(); detector.eval()
    keys = {"watermarked_prob": "prob_watermarked", "clean_prob": "prob_clean", "bit_accuracy": "bit_accuracy",
            "delta_rms": "delta_rms"}
    acc = {k: [] for k in keys}
    classes = []
    for bi, s in enumerate(batches):
        s = s.to(device)
        message = (messages[bi].to(device) if messages is not None else
                   torch.randint(0, 2 ** message_bits, (s.shape[0],), device=device))
        if by_class:
            from .curate import clip_classes
            classes.append(clip_classes(s, SAMPLE_RATE))
        extra = {} if tamper is None else {"tamper": tamper}
        out = eval_forward(generator, detector, s, message, codec=codec, **extra)
        for k, src in keys.items():
            acc[k].append(out[src])
    res = {k: float(torch.cat(v).double().mean()) if v else math.nan for k, v in acc.items()}
    if by_class:
        from .curate import class_report
        res["by_class"] = class_report({k: (torch.cat(v) if v else torch.empty(0)) for k, v in acc.items()},
                                       torch.cat(classes) if classes else torch.empty(0, dtype=torch.int64))
    return res
