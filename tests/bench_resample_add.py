"""The way back of the embed path (a benchmark, not a test):
    python tests/bench_resample_add.py [--seconds 3600] [--channels 2] [--out FILE]
For 48 kHz and 44.1 kHz recordings of `--seconds` and a delta of the same duration at 16 kHz it times, alternating in the same process,
  fused      ops.resample_add(x, delta, rate, out=out): delta resampled to the recording's rate and added to every channel, up kept, one launch;
  fused-noup the same launch with want_up=False;
  composed   what the launch replaces: ops.resample(delta, 16000, rate, out=u) into a preallocated (1, N), then torch.add(x, u, out=out).
Each figure is the median over `--rounds` rounds of a batch of launches sized to at least `--batch-seconds` of device time between two events
(after a warm-up of every shape); the spread is (max - min) / median over the rounds.  Algorithmic bytes: fused 8*C*N + 4*N + 4*n_d
(4*N less without up), composed 8*C*N + 8*N + 4*n_d (up written by one launch and read by the next).  The verdict line compares the fused launch with
the composition against the larger of the two spreads.  Then one whole embed_waveform(x, G, orig_freq=48000, native_rate=True) call on the
host waveform."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import awm_amd                                                        # noqa: E402
from awm_amd import ops                                               # noqa: E402
from bench_timing import batch_ms, launches_for, stats                # noqa: E402

COPY_TBPS = 6.3                                                       # what a plain device copy reaches on this chip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resample_add.py measures on the GPU"
    awm_amd.lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    C = a.channels
    say(f"# {a.seconds} s of {C}-channel audio + delta at 16 kHz; median of {a.rounds} rounds, each >= {a.batch_seconds} s of launches; "
        "spread = (max - min) / median")
    say(f"{'rate':>6} {'code':>10} {'ms':>9} {'spread':>7} {'GB':>6} {'GB/s':>7} {'of copy':>8} {'launches':>8}")
    fused_ms = {}
    for rate in (48000, 44100):
        N = rate * a.seconds
        n_d = ops.resample_length(N, rate, 16000)
        gen = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(C, N, device=dev, generator=gen) * 0.3
        delta = torch.randn(n_d, device=dev, generator=gen) * 0.01
        out = torch.empty(C, N, device=dev)
        nbytes = {"fused": 8 * C * N + 4 * N + 4 * n_d, "fused-noup": 8 * C * N + 4 * n_d, "composed": 8 * C * N + 8 * N + 4 * n_d}

        def fused():
            return ops.resample_add(x, delta, rate, out=out)

        def fused_noup():
            return ops.resample_add(x, delta, rate, out=out, want_up=False)

        L = ops.resample_length(n_d, 16000, rate)                      # >= N (equal for whole seconds): all of delta is resampled, then cut
        u = torch.empty(L, device=dev)

        def composed():
            ops.resample(delta.view(1, -1), 16000, rate, out=u)
            return torch.add(x, u[:N], out=out)

        codes = {"fused": fused, "fused-noup": fused_noup, "composed": composed}
        want = composed().clone()
        got, up = fused()
        same = torch.equal(got, want) and torch.equal(up.view(-1), u[:N]) and torch.equal(fused_noup()[0], want)
        say(f"# {rate}: fused == composed bit for bit: {same}")
        del want, got, up
        n = {k: launches_for(fn, a.batch_seconds, 4000) for k, fn in codes.items()}
        times = {k: [] for k in codes}
        for _ in range(a.rounds):                                     # alternate the codes inside every round
            for k, fn in codes.items():
                times[k].append(batch_ms(fn, n[k]))
        res = {k: stats(times[k]) for k in codes}
        for k in codes:
            med, spread = res[k]
            tbps = nbytes[k] / med / 1e9
            say(f"{rate:6d} {k:>10} {med:9.3f} {100 * spread:6.1f}% {nbytes[k] / 1e9:6.2f} {1e3 * tbps:7.0f} {100 * tbps / COPY_TBPS:7.0f}% {n[k]:8d}")
        slack = max(res["fused"][1], res["composed"][1])
        ok = res["fused"][0] <= res["composed"][0] * (1 + slack)
        say(f"# {rate}: fused / composed = {res['fused'][0] / res['composed'][0]:.3f} (larger spread {100 * slack:.1f}%): "
            f"{'not slower' if ok else 'SLOWER'} than the composition")
        fused_ms[rate] = res["fused"][0]
        del x, delta, out, u
        torch.cuda.empty_cache()

    # ---- the whole embed_waveform(native_rate=True) call for the 48 kHz recording
    G = awm_amd.Generator(16).to(dev).eval()
    N = 48000 * a.seconds
    xh = torch.randn(C, N, generator=torch.Generator().manual_seed(2)) * 0.3
    msgs = torch.randint(0, 2 ** 16, (-(-ops.resample_length(N, 48000, 16000) // 16000),), generator=torch.Generator().manual_seed(3))
    awm_amd.embed_waveform(xh, G, device=dev, messages=msgs, orig_freq=48000, native_rate=True)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        awm_amd.embed_waveform(xh, G, device=dev, messages=msgs, orig_freq=48000, native_rate=True)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    med, spread = stats(ts)
    say(f"# embed_waveform(orig_freq=48000, native_rate=True), waveform on the host: {med:.1f} ms (spread {100 * spread:.1f}% of 3 calls); "
        f"resample_add launch {fused_ms[48000]:.3f} ms = {100 * fused_ms[48000] / med:.2f}% of the call")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
