"""The transform-codec launches (a benchmark, not a test):
    python tests/bench_mdct_codec.py [--hop 256] [--band 8] [--rounds 7] [--out FILE]
It times, alternating in the same process, on x (512, 16000) and (1024, 16000) fp32 with a per-row SNR of 10..30 dB and a 7 kHz cut,
  fwd+codes  wm_mdct_codec with the quantiser on and the int16 codes written (what a "dead_zone" forward does);
  fwd        the same without the codes (a "straight_through" forward, and every no_grad call);
  bwd-st     the backward of "straight_through": the launch with quantise = 0 on dy;
  bwd-dz     the backward of "dead_zone": the same with the forward's codes as mask_in;
  mul        torch.mul(x, 0.7, out=out), a plain pass over the same two frames of bytes;
each as the median over `--rounds` rounds of a batch of launches sized to at least `--batch-seconds` of device time between two events
(after a warm-up), the spread being (max - min) / median over the rounds.  GB/s is against the 8 * rows * n bytes that must move (x read,
y written); the codes (2 bytes per coefficient, (ceil(n / hop) + 1) * hop per row) come on top where they are written or read and are
listed in their own column.  GFLOP/s counts the two products per frame the kernel runs (M x M analysis, M x kcut synthesis: 2 M (M + kcut)
per frame, the shared and the padded frames of every workgroup included)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import awm_amd                                                        # noqa: E402
from awm_amd import ops                                               # noqa: E402
from awm_amd.ops import _stream                                       # noqa: E402
from bench_timing import batch_ms, launches_for, stats                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--band", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mdct_codec.py measures on the GPU"
    lib = awm_amd.lib
    lib.load()
    dev = torch.device("cuda:0")
    M, band = a.hop, a.band
    kcut = ops.mdct_kcut(M, band, 7000)
    fs = ops.mdct_default_floor_step(M)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# hop {M}, band {band}, kcut {kcut}, floor_step {fs:.3e}; median of {a.rounds} rounds, each >= {a.batch_seconds} s of launches; "
        "spread = (max - min) / median")
    say(f"{'shape':>16} {'code':>10} {'us':>9} {'spread':>7} {'MB':>7} {'GB/s':>7} {'codes MB':>8} {'GFLOP/s':>8} {'launches':>8}")
    gen = torch.Generator(device=dev).manual_seed(1)
    for rows, n in ((512, 16000), (1024, 16000)):
        x = 0.1 * torch.randn(rows, n, device=dev, generator=gen)
        dy = torch.randn(rows, n, device=dev, generator=gen)
        snr = 10.0 + 20.0 * torch.rand(rows, device=dev, generator=gen)
        out = torch.empty_like(x)
        F = ops.mdct_frames(n, M)
        codes = torch.empty(rows, F, M, dtype=torch.int16, device=dev)
        px, pdy, pout, pcodes, psnr = (t.data_ptr() for t in (x, dy, out, codes, snr))

        def call(src, codes_out, mask_in, quantise):
            lib.wm_mdct_codec(src, pout, codes_out, mask_in, psnr, rows, n, M, band, kcut, fs, quantise, _stream())
        call(px, pcodes, None, 1)                                     # the codes the dead-zone backward reads
        runs = {
            "fwd+codes": lambda: call(px, pcodes, None, 1),
            "fwd": lambda: call(px, None, None, 1),
            "bwd-st": lambda: call(pdy, None, None, 0),
            "bwd-dz": lambda: call(pdy, None, pcodes, 0),
            "mul": lambda: torch.mul(x, 0.7, out=out),
        }
        extra = {"fwd+codes": 2 * rows * F * M, "fwd": 0, "bwd-st": 0, "bwd-dz": 2 * rows * F * M, "mul": 0}
        width, per_row = ops.mdct_plan(n, M)
        tiles = rows * per_row
        flop = tiles * width * 2.0 * M * (M + kcut)
        k = {c: launches_for(fn, a.batch_seconds, 20000) for c, fn in runs.items()}
        times = {c: [] for c in runs}
        for _ in range(a.rounds):                                     # alternate the codes inside every round
            for c, fn in runs.items():
                times[c].append(batch_ms(fn, k[c]))
        res = {c: stats(v) for c, v in times.items()}
        for c in runs:
            med, spread = res[c]
            mb = 8 * rows * n / 1e6
            gf = "" if c == "mul" else f"{flop / med / 1e6:8.0f}"
            say(f"{f'({rows}, {n})':>16} {c:>10} {1e3 * med:9.2f} {100 * spread:6.1f}% {mb:7.2f} {mb / med:7.0f} {extra[c] / 1e6:8.2f} {gf:>8} "
                f"{k[c]:8d}")
        say(f"# ({rows}, {n}): fwd / mul = {res['fwd'][0] / res['mul'][0]:.1f}, fwd+codes / fwd = {res['fwd+codes'][0] / res['fwd'][0]:.2f}, "
            f"bwd-dz / bwd-st = {res['bwd-dz'][0] / res['bwd-st'][0]:.2f}; {tiles} workgroups of {width} frames for {rows * F} frames")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
