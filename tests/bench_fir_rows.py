"""The reverb launches (a benchmark, not a test):
    python tests/bench_fir_rows.py [--rounds 7] [--out FILE]
It times, alternating in the same process, on x (512, 16000) and (1024, 16000) fp32 with per-row responses of K = 64, 512, 2048, 4096 taps,
  fwd      wm_fir_rows, reverse = 0 (a forward pass of attacks.Reverb / Convolved);
  bwd      wm_fir_rows, reverse = 1 (their backward pass);
  fft      what one would write without the kernel: torch.fft.rfft of x and of the taps at length L = 2^ceil(log2(n + K)), a multiply,
           torch.fft.irfft, the first n samples copied out -- the transform of the taps is part of it, since Reverb draws new taps every call;
  mul      torch.mul(x, 0.7, out=out), a plain pass over the same two frames of bytes: the byte floor;
and once per shape list  rir  wm_rir_synth at (512, 2048), each as the median over `--rounds` rounds of a batch of launches sized to at least
`--batch-seconds` of device time between two events (after a warm-up), the spread being (max - min) / median over the rounds.  GFLOP/s counts
the 2 n K operations per row of the definition (the kernel also multiplies the zero padding of its first and last lag block).  The last line
relates one fwd + one bwd at (256, 16000), K = 2048, to the 48.4 ms of a B = 256 train step on record."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import awm_amd                                                        # noqa: E402
from awm_amd.ops import _stream                                       # noqa: E402
from bench_timing import measure                                      # noqa: E402

STEP_MS = 48.4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--taps", type=int, nargs="+", default=[64, 512, 2048, 4096])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fir_rows.py measures on the GPU"
    lib = awm_amd.lib
    lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# per-row taps; median of {a.rounds} rounds, each >= {a.batch_seconds} s of launches; spread = (max - min) / median")
    say(f"{'shape':>16} {'K':>6} {'code':>5} {'us':>9} {'spread':>7} {'GFLOP/s':>8} {'launches':>8}")
    gen = torch.Generator(device=dev).manual_seed(1)

    def fir_runs(rows, n, K):
        x = torch.randn(rows, n, device=dev, generator=gen)
        dy = torch.randn(rows, n, device=dev, generator=gen)
        h = torch.randn(rows, K, device=dev, generator=gen) * torch.exp(-torch.arange(K, device=dev) * (6.9 / K))
        out = torch.empty_like(x)
        L = 1 << (n + K - 1).bit_length()
        px, pdy, ph, pout = (t.data_ptr() for t in (x, dy, h, out))

        def fft():
            y = torch.fft.irfft(torch.fft.rfft(x, n=L) * torch.fft.rfft(h, n=L), n=L)
            out.copy_(y[:, :n])
        runs = {
            "fwd": lambda: lib.wm_fir_rows(px, ph, pout, rows, n, K, K, 0, _stream()),
            "bwd": lambda: lib.wm_fir_rows(pdy, ph, pout, rows, n, K, K, 1, _stream()),
            "fft": fft,
            "mul": lambda: torch.mul(x, 0.7, out=out),
        }
        # the two agree before they are compared for speed
        runs["fwd"]()
        y = out.clone()
        fft()
        scale = float((x.abs().max() * h.abs().sum(dim=1).max()))
        assert float((y - out).abs().max()) <= 1e-4 * scale, "the kernel and the torch.fft composition disagree"
        return runs

    for rows, n in ((512, 16000), (1024, 16000)):
        for K in a.taps:
            res = measure(fir_runs(rows, n, K), a.rounds, a.batch_seconds)
            for c, (med, spread, k) in res.items():
                gf = "" if c in ("mul", "fft") else f"{2.0 * rows * n * K / med / 1e6:8.0f}"
                say(f"{f'({rows}, {n})':>16} {K:6d} {c:>5} {1e3 * med:9.2f} {100 * spread:6.1f}% {gf:>8} {k:8d}")
            say(f"# ({rows}, {n}) K {K}: fwd / fft = {res['fwd'][0] / res['fft'][0]:.2f}, bwd / fft = {res['bwd'][0] / res['fft'][0]:.2f}, "
                f"fwd / mul = {res['fwd'][0] / res['mul'][0]:.1f}")
    rows, K = 512, 2048
    params = torch.tensor([[0.3, 6.0]], device=dev).repeat(rows, 1)
    hs = torch.empty(rows, K, device=dev)
    res = measure({"rir": lambda: lib.wm_rir_synth(params.data_ptr(), hs.data_ptr(), rows, K, 16000.0, 0, 1, 0, _stream())}, a.rounds,
                  a.batch_seconds)
    med, spread, k = res["rir"]
    say(f"{f'({rows}, {K})':>16} {K:6d} {'rir':>5} {1e3 * med:9.2f} {100 * spread:6.1f}% {'':>8} {k:8d}")
    res = measure({c: fn for c, fn in fir_runs(256, 16000, 2048).items() if c in ("fwd", "bwd")}, a.rounds, a.batch_seconds)
    both = res["fwd"][0] + res["bwd"][0]
    say(f"# (256, 16000) K 2048: fwd {1e3 * res['fwd'][0]:.2f} us + bwd {1e3 * res['bwd'][0]:.2f} us = {100 * both / STEP_MS:.2f} % of the "
        f"{STEP_MS} ms B = 256 train step on record")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
