"""The biquad / 16-bit PCM codec launch and the device save path (a benchmark, not a test):
    python tests/bench_biquad.py [--batch 256] [--seconds 60] [--out FILE]
It times, alternating in the same process,
  codec      ops.biquad(x, coeffs, mode="round", out=out) on x [batch, 1, 16000]: main15c's perceptual_postprocess, one launch;
  codec-mask the same launch with mask_out=True (the forward of grad="straight_through");
  adjoint    its backward: the reverse launch with mask_in;
  add        torch.add(x, y, out=out) over the same three frames of bytes -- the launch streams one frame in and one out, so the add,
             which moves three, is its ceiling: a streaming kernel cannot be expected to beat it by more than 3/2;
each as the median over `--rounds` rounds of a batch of launches sized to at least `--batch-seconds` of device time between two events
(after a warm-up), the spread being (max - min) / median over the rounds.  Algorithmic bytes: codec 8 per sample, add 12.
Then save_audio(device="cuda") against save_audio(device=None) -- the host path: float32 download, scipy's lfilter on one core, the
int16 cast -- for a `--channels`-channel, `--seconds`-second, 48 kHz CUDA waveform: wall clock of the whole call, synchronised on both
sides, the median of `--save-rounds` calls each, alternating; and the encode_pcm16 launch of that waveform alone."""
import argparse
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import awm_amd                                                        # noqa: E402
from awm_amd import ops                                               # noqa: E402
from bench_timing import batch_ms, launches_for, stats                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--save-rounds", type=int, default=5)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_biquad.py measures on the GPU"
    awm_amd.lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, T = a.batch, 16000
    coeffs = ops.biquad_lowpass_coeffs(16000, 7000)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, 1, T, device=dev, generator=gen) * 0.3
    y = torch.randn(B, 1, T, device=dev, generator=gen) * 0.01
    out = torch.empty_like(x)
    _, mask = ops.biquad(x, coeffs, mode="round", mask_out=True)
    codes = {
        "codec": lambda: ops.biquad(x, coeffs, mode="round", out=out),
        "codec-mask": lambda: ops.biquad(x, coeffs, mode="round", mask_out=True, out=out),
        "adjoint": lambda: ops.biquad(y, coeffs, clamp=False, reverse=True, mask_in=mask, out=out),
        "add": lambda: torch.add(x, y, out=out),
    }
    nbytes = {"codec": 8 * B * T, "codec-mask": 8 * B * T + B * T // 8, "adjoint": 8 * B * T + B * T // 8, "add": 12 * B * T}
    say(f"# [{B},1,{T}] fp32, 16 kHz / 7 kHz section, warm-up {ops.biquad_plan(coeffs)[0]} samples; median of {a.rounds} rounds, each >= "
        f"{a.batch_seconds} s of launches; spread = (max - min) / median")
    say(f"{'code':>10} {'us':>9} {'spread':>7} {'MB':>7} {'GB/s':>7} {'launches':>8}")
    n = {k: launches_for(fn, a.batch_seconds, 20000) for k, fn in codes.items()}
    times = {k: [] for k in codes}
    for _ in range(a.rounds):                                         # alternate the codes inside every round
        for k, fn in codes.items():
            times[k].append(batch_ms(fn, n[k]))
    res = {k: stats(times[k]) for k in codes}
    for k in codes:
        med, spread = res[k]
        say(f"{k:>10} {1e3 * med:9.2f} {100 * spread:6.1f}% {nbytes[k] / 1e6:7.2f} {nbytes[k] / med / 1e6:7.0f} {n[k]:8d}")
    say(f"# codec / add = {res['codec'][0] / res['add'][0]:.2f} (spreads {100 * res['codec'][1]:.1f}% / {100 * res['add'][1]:.1f}%)")

    # ---- the save path of a device-resident waveform
    C, rate = a.channels, 48000
    N = rate * a.seconds
    w = torch.randn(C, N, device=dev, generator=gen) * 0.3
    enc = lambda: awm_amd.encode_pcm16(w, rate)                       # noqa: E731
    k = launches_for(enc, a.batch_seconds, 2000)
    med, spread = stats([batch_ms(enc, k) for _ in range(a.rounds)])
    say(f"# encode_pcm16 launch, ({C}, {N}) at {rate} Hz: {1e3 * med:.1f} us (spread {100 * spread:.1f}%, {k} launches a round), "
        f"{6 * C * N / med / 1e6:.0f} GB/s of 6 bytes a sample")
    with tempfile.TemporaryDirectory() as d:
        paths = {"cuda": os.path.join(d, "gpu.wav"), None: os.path.join(d, "host.wav")}
        ts = {"cuda": [], None: []}
        for r in range(a.save_rounds + 1):                            # the first round of both is the warm-up
            for device in ("cuda", None):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                awm_amd.save_audio(w, paths[device], rate, device=device)
                torch.cuda.synchronize()
                if r:
                    ts[device].append((time.perf_counter() - t0) * 1e3)
        g, h = stats(ts["cuda"]), stats(ts[None])
        import numpy as np
        import wave
        frames = []
        for p in paths.values():
            with wave.open(p, "rb") as f:
                frames.append(np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").astype(np.int64))
        diff = np.abs(frames[0] - frames[1])
    say(f"# save_audio, ({C}, {N}) CUDA waveform at {rate} Hz, whole call incl. writing the file, median of {a.save_rounds}:")
    say(f"#   device=\"cuda\" {g[0]:9.1f} ms (spread {100 * g[1]:.1f}%)")
    say(f"#   device=None   {h[0]:9.1f} ms (spread {100 * h[1]:.1f}%)   host / device = {h[0] / g[0]:.1f}")
    say(f"#   codes of the two files: max |difference| {int(diff.max())}, {100 * float((diff != 0).mean()):.3f}% of the samples differ")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
