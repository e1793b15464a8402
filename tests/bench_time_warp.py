"""The time-warp launches (a benchmark, not a test):
    python tests/bench_time_warp.py [--rounds 7] [--out FILE]
It times, alternating in the same process, on x (512, 16000) fp32 with the default 16 x 512 table,
  fwd      wm_time_warp, adjoint = 0 (a forward pass of attacks.TimeWarp);
  adj      wm_time_warp, adjoint = 1 (its backward pass);
  mul      torch.mul(x, 0.7, out=out), a plain pass over the same two frames of bytes: the byte floor as measured;
for every row at speed 1 (c = 1: 32 or 33 taps a sample), every row at speed 2 (c = 1/2: 64 or 65 taps), and the default module's draw
(speed uniform in [0.9, 1.1] per row, no flutter), then
  module   attacks.TimeWarp() called on (512, 1, 16000): the draw on the host, its copy to the device and the forward launch;
  resamp   attacks.Resampled(8000) on the same tensor, the round trip profiles/bench_resample_rows_b512.txt records;
each as the median over `--rounds` rounds of a batch of launches sized to at least `--batch-seconds` of device time between two events
(after a warm-up), the spread being (max - min) / median over the rounds.  `x floor` is the time over the launch's HBM floor, 2 * 4 * rows * n
bytes at the 6.3 TB/s a plain copy reaches; Gtap/s counts rows * n * taps weights of the definition."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import awm_amd                                                        # noqa: E402
from awm_amd import attacks, ops                                      # noqa: E402
from awm_amd.ops import _stream                                       # noqa: E402
from bench_timing import measure                                      # noqa: E402

COPY_TBS = 6.3
RESAMPLED_MS = 0.0483                                                 # profiles/bench_resample_rows_b512.txt, `forward`


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_time_warp.py measures on the GPU"
    lib = awm_amd.lib
    lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rows, n, Z, R = 512, 16000, 16, 512
    floor_ms = 2 * 4 * rows * n / (COPY_TBS * 1e12) * 1e3
    say(f"# x ({rows}, {n}), table {Z} x {R}; median of {a.rounds} rounds, each >= {a.batch_seconds} s of launches; spread = (max - min) / median")
    say(f"# HBM floor {1e3 * floor_ms:.2f} us = {2 * 4 * rows * n / 1e6:.1f} MB at {COPY_TBS} TB/s; Resampled(8000) round trip on record {1e3 * RESAMPLED_MS:.1f} us")
    say(f"{'params':>10} {'code':>6} {'us':>9} {'spread':>7} {'x floor':>8} {'x resamp':>8} {'Gtap/s':>8} {'launches':>8}")
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(rows, n, device=dev, generator=gen)
    dy = torch.randn(rows, n, device=dev, generator=gen)
    out = torch.empty_like(x)
    tab = ops.time_warp_table(Z, R).to(dev)
    module = awm_amd.TimeWarp()
    sets = {
        "speed 1": (torch.tensor([[1.0, 0, 0, 0, 0, 1.0]]).repeat(rows, 1), 32.0),
        "speed 2": (torch.tensor([[2.0, 0, 0, 0, 0, 0.5]]).repeat(rows, 1), 64.0),
        "default": (torch.from_numpy(attacks.row_warp_params(0, 0, range(rows), module.speed, module.shift_s, None, None, 16000)), None),
    }
    for name, (params, taps) in sets.items():
        taps = float((2 * Z / params[:, 5].double()).mean()) if taps is None else taps
        params = params.to(dev)
        px, pdy, pp, pt, po = (t.data_ptr() for t in (x, dy, params, tab, out))
        runs = {
            "fwd": lambda: lib.wm_time_warp(px, pp, pt, po, rows, n, Z, R, 0, _stream()),
            "adj": lambda: lib.wm_time_warp(pdy, pp, pt, po, rows, n, Z, R, 1, _stream()),
            "mul": lambda: torch.mul(x, 0.7, out=out),
        }
        if name == "speed 1":                                         # the identity before it is timed
            runs["fwd"]()
            assert torch.equal(out, x), "speed 1 is not the identity"
        res = measure(runs, a.rounds, a.batch_seconds)
        for c, (med, spread, k) in res.items():
            gt = "" if c == "mul" else f"{rows * n * taps / med / 1e6:8.1f}"
            say(f"{name:>10} {c:>6} {1e3 * med:9.2f} {100 * spread:6.1f}% {med / floor_ms:8.1f} {med / RESAMPLED_MS:8.2f} {gt:>8} {k:8d}")
    x3 = x.view(rows, 1, n)
    resampled = awm_amd.Resampled(8000)
    res = measure({"module": lambda: module(x3), "resamp": lambda: resampled(x3)}, a.rounds, a.batch_seconds)
    for c, (med, spread, k) in res.items():
        say(f"{'(512,1,T)':>10} {c:>6} {1e3 * med:9.2f} {100 * spread:6.1f}% {med / floor_ms:8.1f} {med / RESAMPLED_MS:8.2f} {'':>8} {k:8d}")
    say(f"# module / resamp in this run = {res['module'][0] / res['resamp'][0]:.2f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
