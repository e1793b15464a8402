"""Sample-rate conversion of the file ingest (a benchmark, not a test):
    python tests/bench_resample.py [--seconds 3600] [--channels 2] [--out FILE]
For 48 kHz and 44.1 kHz recordings of `--seconds` it times, alternating in the same process,
  kernel    ops.resample(x, rate, 16000, seg_len=16000): channel mean + resampling + segment padding, one launch;
  conv1d    what a torchaudio user runs on the same GPU for the resampling alone: F.conv1d of the zero-padded, already channel-averaged
            input with the dense (Q, 1, K) table at stride P (torchaudio.functional.resample's own formulation);
  pipeline  the conv1d with everything around it that the kernel also does: mean over channels, F.pad, the (phase, period) transpose, the cut
            to L samples and the zero-padded segment tail.
Each figure is the median over `--rounds` rounds of a batch of launches sized to at least `--batch-seconds` of device time between two events
(after a warm-up of every shape); the spread is (max - min) / median over the rounds.  Algorithmic bytes: 4*C*N read + 4*S*16000 written.
Then one whole detect_waveform(x, D, orig_freq=48000) call on the host waveform, and on a waveform that already lies on the device."""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import awm_amd                                                        # noqa: E402
from awm_amd import ops                                               # noqa: E402
from bench_timing import batch_ms, launches_for, stats                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resample.py measures on the GPU"
    awm_amd.lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    C = a.channels
    say(f"# {a.seconds} s of {C}-channel audio to 16 kHz; median of {a.rounds} rounds, each >= {a.batch_seconds} s of launches; spread = (max - min) / median")
    say(f"{'rate':>6} {'code':>9} {'ms':>9} {'spread':>7} {'GB/s':>7} {'launches':>8}")
    kernel_ms = {}
    for rate in (48000, 44100):
        N = rate * a.seconds
        x = torch.randn(C, N, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.3
        tab = ops.resample_table(rate, 16000)
        P, Q, width = tab["P"], tab["Q"], tab["width"]
        L = ops.resample_length(N, rate, 16000)
        S = -(-L // 16000)
        out = torch.empty(S * 16000, device=dev)
        dense = tab["dense"].to(dev)[:, None, :]
        mono_padded = F.pad(x.mean(dim=0, keepdim=True), (width, width + P))[None]
        nbytes = 4 * C * N + 4 * S * 16000

        def kernel():
            return ops.resample(x, rate, 16000, seg_len=16000, out=out)

        def conv():
            return F.conv1d(mono_padded, dense, stride=P)

        def pipeline():
            m = F.pad(x.mean(dim=0, keepdim=True), (width, width + P))[None]
            y = F.conv1d(m, dense, stride=P).transpose(1, 2).reshape(-1)[:L]
            return F.pad(y, (0, S * 16000 - L)).view(S, 1, 16000)

        codes = {"kernel": kernel}
        for name, fn in (("conv1d", conv), ("pipeline", pipeline)):
            try:
                fn()
                torch.cuda.synchronize()
                codes[name] = fn
            except Exception as e:                                    # the library may refuse a 10^8-sample row: say so, do not hide it
                say(f"{rate:6d} {name:>9} failed: {type(e).__name__}: {str(e)[:120]}")
        ref = pipeline() if "pipeline" in codes else None
        if ref is not None:
            d = (kernel() - ref).abs().max().item()
            say(f"# {rate}: max |kernel - conv1d pipeline| = {d:.3e}")
            del ref
        n = {k: launches_for(fn, a.batch_seconds, 4000) for k, fn in codes.items()}
        times = {k: [] for k in codes}
        for _ in range(a.rounds):                                     # alternate the codes inside every round
            for k, fn in codes.items():
                times[k].append(batch_ms(fn, n[k]))
        for k in codes:
            med, spread = stats(times[k])
            say(f"{rate:6d} {k:>9} {med:9.3f} {100 * spread:6.1f}% {nbytes / med / 1e6:7.0f} {n[k]:8d}")
        kernel_ms[rate] = stats(times["kernel"])[0]
        del x, out, mono_padded
        torch.cuda.empty_cache()

    # ---- the whole detect_waveform call for the 48 kHz recording
    D = awm_amd.Detector(16).to(dev).eval()
    N = 48000 * a.seconds
    xh = torch.randn(C, N, generator=torch.Generator().manual_seed(2)) * 0.3
    for where, xin in (("host", xh), ("device", xh.to(dev))):
        awm_amd.detect_waveform(xin, D, device=dev, orig_freq=48000)
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            awm_amd.detect_waveform(xin, D, device=dev, orig_freq=48000)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        med, spread = stats(ts)
        say(f"# detect_waveform(orig_freq=48000), waveform on the {where}: {med:.1f} ms (spread {100 * spread:.1f}% of 3 calls); "
            f"resampling kernel {kernel_ms[48000]:.3f} ms = {100 * kernel_ms[48000] / med:.2f}% of the call")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
