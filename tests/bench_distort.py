"""The channel-distortion launches (a benchmark, not a test):
    python tests/bench_distort.py [--batch 512] [--rounds 7] [--out FILE]
It times, alternating in the same process, on x [batch, 1, 16000] fp32 and on one (1, 10^7) row,
  noise      wm_distort with gain (-6, 6) dB and noise at (20, 40) dB on every row: the row sums, then g x + s z with z generated in the kernel;
  gain       the same call with p_noise = 0: the row sums and g x (no generator);
  bwd        wm_distort_bwd, noise_grad "through": sum dy z (z generated again), then g dy + k x;
  bwd-det    wm_distort_bwd, "detached": g dy alone;
  mul        torch.mul(x, 0.7, out=out), the plain y = g x pass over the same two frames of bytes;
each as the median over `--rounds` rounds of a batch of launches sized to at least `--batch-seconds` of device time between two events
(after a warm-up), the spread being (max - min) / median over the rounds.  Algorithmic bytes: noise and gain read x twice and write y (12 per
sample), bwd reads dy twice and x once and writes dx (16), bwd-det and mul 8."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import awm_amd                                                        # noqa: E402
from awm_amd.ops import _stream                                       # noqa: E402
from bench_timing import batch_ms, launches_for, stats                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_distort.py measures on the GPU"
    lib = awm_amd.lib
    lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# median of {a.rounds} rounds, each >= {a.batch_seconds} s of launches; spread = (max - min) / median")
    say(f"{'shape':>16} {'code':>8} {'us':>9} {'spread':>7} {'MB':>7} {'GB/s':>7} {'launches':>8}")
    gen = torch.Generator(device=dev).manual_seed(1)
    for rows, n in ((a.batch, 16000), (1, 10 ** 7)):
        x = torch.randn(rows, n, device=dev, generator=gen) * 0.3
        dy = torch.randn(rows, n, device=dev, generator=gen)
        out, stat, stat_gain = torch.empty_like(x), torch.empty(rows, 4, device=dev), torch.empty(rows, 4, device=dev)
        need = ctypes.c_longlong(0)
        lib.wm_distort_plan(rows, n, ctypes.addressof(need), None)
        scratch = torch.empty(need.value, device=dev)
        px, pdy, pout, pscratch = (t.data_ptr() for t in (x, dy, out, scratch))

        def fwd(p_noise, st):
            lib.wm_distort(px, pout, st.data_ptr(), pscratch, rows, n, 0, 1234, 0, -6.0, 6.0, 20.0, 40.0, p_noise, _stream())

        def bwd(through):
            lib.wm_distort_bwd(pdy, px, stat.data_ptr(), pout, pscratch, rows, n, 0, 1234, 0, through, _stream())
        fwd(1.0, stat)                                                # the stat the backward calls read
        codes = {
            "noise": lambda: fwd(1.0, stat),
            "gain": lambda: fwd(0.0, stat_gain),
            "bwd": lambda: bwd(1),
            "bwd-det": lambda: bwd(0),
            "mul": lambda: torch.mul(x, 0.7, out=out),
        }
        nbytes = {"noise": 12, "gain": 12, "bwd": 16, "bwd-det": 8, "mul": 8}
        k = {c: launches_for(fn, a.batch_seconds, 20000) for c, fn in codes.items()}
        times = {c: [] for c in codes}
        for _ in range(a.rounds):                                     # alternate the codes inside every round
            for c, fn in codes.items():
                times[c].append(batch_ms(fn, k[c]))
        res = {c: stats(v) for c, v in times.items()}
        for c in codes:
            med, spread = res[c]
            mb = nbytes[c] * rows * n / 1e6
            say(f"{f'({rows}, {n})':>16} {c:>8} {1e3 * med:9.2f} {100 * spread:6.1f}% {mb:7.2f} {mb / med:7.0f} {k[c]:8d}")
        say(f"# ({rows}, {n}): noise / mul = {res['noise'][0] / res['mul'][0]:.2f}, gain / mul = {res['gain'][0] / res['mul'][0]:.2f} "
            f"(spreads {100 * res['noise'][1]:.1f}% / {100 * res['gain'][1]:.1f}% / {100 * res['mul'][1]:.1f}%); "
            f"noise: {rows * n / res['noise'][0] / 1e6:.2f} G samples/s")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
