"""The time-stretch launches (a benchmark, not a test):
    python tests/bench_wsola.py [--rounds 7] [--out FILE]
It times, alternating in the same process, on x (512, 16000) fp32 at the default frame and search range (L = 512, S = 128),
  search   wm_wsola, mode 0 (a forward pass of attacks.TimeStretch: the search, the offsets and the synthesis);
  synth    wm_wsola, mode 1 (the synthesis alone, from the offsets the search left);
  adj      wm_wsola, mode 2 (the backward pass);
  mul      torch.mul(x, 0.7, out=out), a plain pass over the same two frames of bytes: the byte floor as measured;
on noise and on speech-like rows (harmonics of a gliding fundamental plus noise), for every row at rate 1, every row at rate 1.25 and the
default module's draw (rate uniform in [0.9, 1.1] per row), then
  stretch  attacks.TimeStretch() called on (512, 1, 16000): the draw on the host, its copy to the device and the forward launch;
  pitch    attacks.PitchShift() on the same tensor: the draw, the stretch to the longest row's length, the cut at every row's own length and
           the wm_time_warp launch;
  warp     attacks.TimeWarp() on the same tensor, the module profiles/bench_time_warp_b512.txt records;
each as the median over `--rounds` rounds of a batch of launches sized to at least `--batch-seconds` of device time between two events
(after a warm-up), the spread being (max - min) / median over the rounds.  `x floor` is the time over the launch's HBM floor, 2 * 4 * rows * n
bytes at the 6.3 TB/s a plain copy reaches; Gterm/s counts the rows * (K - 1) * (2 S + 1) * L squared differences of
the definition's search (K - 1 searched frames a row)."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import awm_amd                                                        # noqa: E402
from awm_amd import attacks, ops                                      # noqa: E402
from awm_amd.ops import _stream                                       # noqa: E402
from bench_timing import measure                                      # noqa: E402

COPY_TBS = 6.3


def speech_like(rows, n, dev, gen):
    """ten harmonics of a fundamental gliding between 90 and 250 Hz at 16 kHz, plus noise 26 dB below"""
    t = torch.arange(n, device=dev, dtype=torch.float64) / 16000.0
    f0 = 90 + 160 * torch.rand(rows, 1, device=dev, generator=gen, dtype=torch.float64)
    glide = 80 * torch.rand(rows, 1, device=dev, generator=gen, dtype=torch.float64) - 40
    phase = 2 * math.pi * (f0 * t + 0.5 * glide * t * t)
    x = sum(torch.sin(h * phase + 2 * math.pi * torch.rand(rows, 1, device=dev, generator=gen, dtype=torch.float64)) / h for h in range(1, 11))
    return (0.5 * x).float() + 0.05 * torch.randn(rows, n, device=dev, generator=gen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_wsola.py measures on the GPU"
    lib = awm_amd.lib
    lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rows, n, L, S = 512, 16000, 512, 128
    K = ops.wsola_frames(n, L)
    terms = rows * (K - 1) * (2 * S + 1) * L
    floor_ms = 2 * 4 * rows * n / (COPY_TBS * 1e12) * 1e3
    say(f"# x ({rows}, {n}), L {L}, S {S}: K = {K} frames a row; median of {a.rounds} rounds, each >= {a.batch_seconds} s of launches; "
        "spread = (max - min) / median")
    say(f"# HBM floor {1e3 * floor_ms:.2f} us = {2 * 4 * rows * n / 1e6:.1f} MB at {COPY_TBS} TB/s; the search is (K - 1) (2 S + 1) L = "
        f"{(K - 1) * (2 * S + 1) * L / 1e6:.2f} M squared differences a row, {terms / 1e9:.2f} G a launch")
    say(f"{'data':>7} {'rate':>8} {'code':>7} {'us':>9} {'spread':>7} {'x floor':>8} {'Gterm/s':>8} {'launches':>8}")
    gen = torch.Generator(device=dev).manual_seed(1)
    data = {"noise": torch.randn(rows, n, device=dev, generator=gen), "speech": speech_like(rows, n, dev, gen)}
    dy = torch.randn(rows, n, device=dev, generator=gen)
    out = torch.empty(rows, n, device=dev)
    delta = torch.empty(rows, K, dtype=torch.int32, device=dev)
    win = ops.wsola_window(L).to(dev)
    module = awm_amd.TimeStretch()
    sets = {"1": torch.full((rows,), 1.0), "1.25": torch.full((rows,), 1.25),
            "default": torch.from_numpy(attacks.row_stretch_rates(0, 0, range(rows), module.rate))}
    for dname, x in data.items():
        for name, rate in sets.items():
            rate = rate.to(dev)
            px, pdy, pr, pw, po, pd = (t.data_ptr() for t in (x, dy, rate, win, out, delta))
            runs = {
                "search": lambda: lib.wm_wsola(px, pr, pw, po, pd, rows, n, n, L, S, 0, _stream()),
                "synth": lambda: lib.wm_wsola(px, pr, pw, po, pd, rows, n, n, L, S, 1, _stream()),
                "adj": lambda: lib.wm_wsola(pdy, pr, pw, po, pd, rows, n, n, L, S, 2, _stream()),
                "mul": lambda: torch.mul(x, 0.7, out=out),
            }
            runs["search"]()                                          # the offsets the other two modes read
            if name == "1":                                           # the identity before it is timed
                assert torch.equal(out, x) and not bool(delta.any()), "rate 1 is not the identity"
            res = measure(runs, a.rounds, a.batch_seconds)
            for c, (med, spread, k) in res.items():
                gt = f"{terms / med / 1e6:8.1f}" if c == "search" else ""
                say(f"{dname:>7} {name:>8} {c:>7} {1e3 * med:9.2f} {100 * spread:6.1f}% {med / floor_ms:8.1f} {gt:>8} {k:8d}")
    x3 = data["speech"].view(rows, 1, n)
    pitch, warp = awm_amd.PitchShift(), awm_amd.TimeWarp()
    res = measure({"stretch": lambda: module(x3), "pitch": lambda: pitch(x3), "warp": lambda: warp(x3)}, a.rounds, a.batch_seconds)
    for c, (med, spread, k) in res.items():
        say(f"{'speech':>7} {'(512,1,T)':>8} {c:>7} {1e3 * med:9.2f} {100 * spread:6.1f}% {med / floor_ms:8.1f} {'':>8} {k:8d}")
    say(f"# stretch / warp in this run = {res['stretch'][0] / res['warp'][0]:.2f}, pitch / warp = {res['pitch'][0] / res['warp'][0]:.2f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
