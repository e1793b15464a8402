"""The resampling attack on a training batch (a benchmark, not a test):
    python tests/bench_resample_rows.py [--batch 512] [--samples 16000] [--rate 8000] [--out FILE]
On a (batch, 1, samples) batch at 16 kHz it times, alternating in the same process,
  forward    attacks.Resampled(rate)(x) under no_grad: two wm_resample_rows launches (down, up);
  fwd+bwd    the same with a backward pass, (y * g).sum().backward(): four launches of the kernel, two of them with the transposed tables,
             plus what autograd adds around them (the product, the sum and their backward are timed too);
  row loop   what a user could do without the batched kernel: ops.resample, one recording per launch, row by row down and up and the cut
             to `samples` -- 2 * batch launches, forward only (that path has no backward).
Each figure is the median over `--rounds` rounds of a batch of calls sized to at least `--batch-seconds` of device time between two events
(after a warm-up); the spread is (max - min) / median over the rounds.  Algorithmic bytes of one forward: each leg reads its input and
writes its output once, 4 * batch * (2 * samples + 2 * L1) with L1 = ceil(rate * samples / 16000); forward + backward moves twice that."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import awm_amd                                                        # noqa: E402
from awm_amd import ops                                               # noqa: E402
from bench_timing import batch_ms, launches_for, stats                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--rate", type=int, default=8000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resample_rows.py measures on the GPU"
    awm_amd.lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, T, rate, sr = a.batch, a.samples, a.rate, 16000
    L1 = ops.resample_length(T, sr, rate)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, 1, T, device=dev, generator=gen) * 0.3
    g = torch.randn(B, 1, T, device=dev, generator=gen)
    att = awm_amd.Resampled(rate)
    fwd_bytes = 4 * B * (2 * T + 2 * L1)

    def forward():
        with torch.no_grad():
            return att(x)

    def forward_backward():
        xg = x.detach().requires_grad_()
        (att(xg) * g).sum().backward()
        return xg.grad

    def row_loop():
        out = torch.empty(B, 1, T, device=dev)
        for r in range(B):
            out[r] = ops.resample(ops.resample(x[r], sr, rate), rate, sr)[:, :T]
        return out

    same = torch.equal(forward(), row_loop())
    say(f"# Resampled({rate}) on ({B}, 1, {T}); median of {a.rounds} rounds, each >= {a.batch_seconds} s of calls; spread = (max - min) / median")
    say(f"# batched result == row loop result, bit for bit: {same}")
    say(f"# compact tables: down {ops.resample_table(sr, rate)['W']} taps x {ops.resample_table(sr, rate)['Q']} phases, "
        f"up {ops.resample_table(rate, sr)['W']} x {ops.resample_table(rate, sr)['Q']}; tile periods down / up: "
        f"{ops.resample_tile_periods(sr, rate)} / {ops.resample_tile_periods(rate, sr)}")
    say(f"{'code':>9} {'ms':>9} {'spread':>7} {'GB/s':>7} {'launches':>8} {'calls':>6}")
    codes = {"forward": (forward, fwd_bytes, 2), "fwd+bwd": (forward_backward, 2 * fwd_bytes, 4), "row loop": (row_loop, fwd_bytes, 2 * B)}
    n = {k: launches_for(fn, a.batch_seconds, 4000) for k, (fn, _, _) in codes.items()}
    times = {k: [] for k in codes}
    for _ in range(a.rounds):                                         # alternate the codes inside every round
        for k, (fn, _, _) in codes.items():
            times[k].append(batch_ms(fn, n[k]))
    for k, (_, nbytes, launches) in codes.items():
        med, spread = stats(times[k])
        say(f"{k:>9} {med:9.4f} {100 * spread:6.1f}% {nbytes / med / 1e6:7.0f} {launches:8d} {n[k]:6d}")
    say(f"# row loop / forward = {stats(times['row loop'])[0] / stats(times['forward'])[0]:.1f}x")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
