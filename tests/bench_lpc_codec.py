"""The predictive-codec launches (a benchmark, not a test):
    python tests/bench_lpc_codec.py [--frame 320] [--order 16] [--rounds 7] [--out FILE]
It times, alternating in the same process, on x (256, 16000) and (512, 16000) fp32 (speech-like rows: white noise through three
resonators) with a per-row SNR of 10..30 dB,
  fwd        wm_lpc_codec with analysis and quantiser (a "straight_through" forward, and every no_grad call);
  fwd+out    the same with the coefficients and the int16 codes written (what a "dead_zone" forward does);
  fwd-given  the forward at given coefficients: no autocorrelation, no Levinson-Durbin (how much of fwd is analysis);
  bwd-dz     the backward of "dead_zone": the adjoint launch with the forward's coefficients and codes;
  mdct       wm_mdct_codec (hop 256, band 8, no cut) on the same x, for scale;
  mul        torch.mul(x, 0.7, out=out), a plain pass over the same bytes;
each as the median over `--rounds` rounds of a batch of launches sized to at least `--batch-seconds` of device time between two events
(after a warm-up), the spread being (max - min) / median over the rounds.
The recursion is the critical path: one workgroup per row runs n dependent steps, so `ns/sample` = time / n is what one step costs a
row while every row of the launch runs beside it, and `cyc@2.4` is that at the 2.4 GHz peak engine clock (the clock is not read: at a
lower real clock the true cycle count is lower in proportion).  The model next to it: a step issues 16 v_fma_f32 in one wave, 4 cycles
each when the wave is alone on its SIMD = 64 cycles, plus the LDS reads and writes of a sixteen-sample block (about 10 instructions,
under one per sample)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import awm_amd                                                        # noqa: E402
from awm_amd import ops                                               # noqa: E402
from awm_amd.ops import _stream                                       # noqa: E402
from bench_timing import batch_ms, launches_for, stats                # noqa: E402


def speech_like(rows, n, dev, gen):
    """white noise through three two-pole resonators (500, 1500, 2500 Hz), peak 0.3: rows with a real spectral envelope"""
    x = torch.randn(rows, n + 200, device=dev, generator=gen, dtype=torch.float64)
    import math
    for fc, bw in ((500.0, 80.0), (1500.0, 120.0), (2500.0, 160.0)):
        rad = math.exp(-math.pi * bw / 16000.0)
        c1, c2 = 2.0 * rad * math.cos(2.0 * math.pi * fc / 16000.0), -rad * rad
        y = torch.zeros(rows, n + 202, device=dev, dtype=torch.float64)
        for t in range(n + 200):
            y[:, t + 2] = x[:, t] + c1 * y[:, t + 1] + c2 * y[:, t]
        x = y[:, 2:]
    x = x[:, 200:]
    return (0.3 * x / x.abs().amax(dim=1, keepdim=True)).float().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", type=int, default=320)
    ap.add_argument("--order", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lpc_codec.py measures on the GPU"
    lib = awm_amd.lib
    lib.load()
    dev = torch.device("cuda:0")
    L, p, fs = a.frame, a.order, ops.LPC_FLOOR_STEP
    M, band = 256, 8
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# frame {L}, order {p}, floor_step {fs:.3e}; median of {a.rounds} rounds, each >= {a.batch_seconds} s of launches; "
        "spread = (max - min) / median; cyc@2.4 = ns/sample * 2.4")
    say(f"{'shape':>16} {'code':>10} {'us':>9} {'spread':>7} {'ns/sample':>10} {'cyc@2.4':>8} {'launches':>8}")
    gen = torch.Generator(device=dev).manual_seed(1)
    lag, expand = (t.to(dev) for t in ops.lpc_tables(p))
    base = speech_like(512, 16000, "cpu", torch.Generator().manual_seed(1)).to(dev)          # 48 600 sequential steps: on the host
    for rows, n in ((256, 16000), (512, 16000)):
        x = base[:rows].contiguous()
        dy = torch.randn(rows, n, device=dev, generator=gen)
        snr = 10.0 + 20.0 * torch.rand(rows, device=dev, generator=gen)
        out = torch.empty_like(x)
        F = ops.lpc_frames(n, L)
        coeffs = torch.empty(rows, F, p, device=dev)
        codes = torch.empty(rows, n, dtype=torch.int16, device=dev)
        px, pdy, pout, pco, pq, psnr, plag, pex = (t.data_ptr() for t in (x, dy, out, coeffs, codes, snr, lag, expand))

        def call(src, cin, cout, qout, mask, quantise, adjoint):
            lib.wm_lpc_codec(src, pout, cin, cout, qout, mask, psnr, plag, pex, rows, n, L, p, fs, quantise, adjoint, _stream())
        call(px, None, pco, pq, None, 1, 0)                           # the coefficients and codes the other launches read
        torch.cuda.synchronize()
        zero_share = float((codes == 0).float().mean())
        runs = {
            "fwd": lambda: call(px, None, None, None, None, 1, 0),
            "fwd+out": lambda: call(px, None, pco, pq, None, 1, 0),
            "fwd-given": lambda: call(px, pco, None, None, None, 1, 0),
            "bwd-dz": lambda: call(pdy, pco, None, None, pq, 0, 1),
            "mdct": lambda: lib.wm_mdct_codec(px, pout, None, None, psnr, rows, n, M, band, M, ops.mdct_default_floor_step(M), 1, _stream()),
            "mul": lambda: torch.mul(x, 0.7, out=out),
        }
        k = {c: launches_for(fn, a.batch_seconds, 20000) for c, fn in runs.items()}
        times = {c: [] for c in runs}
        for _ in range(a.rounds):                                     # alternate the codes inside every round
            for c, fn in runs.items():
                times[c].append(batch_ms(fn, k[c]))
        res = {c: stats(v) for c, v in times.items()}
        for c in runs:
            med, spread = res[c]
            ns = 1e6 * med / n
            rec = f"{ns:10.2f} {2.4 * ns:8.1f}" if c in ("fwd", "fwd+out", "fwd-given", "bwd-dz") else f"{'':>10} {'':>8}"
            say(f"{f'({rows}, {n})':>16} {c:>10} {1e3 * med:9.2f} {100 * spread:6.1f}% {rec} {k[c]:8d}")
        say(f"# ({rows}, {n}): fwd / mdct = {res['fwd'][0] / res['mdct'][0]:.1f}, fwd / fwd-given = {res['fwd'][0] / res['fwd-given'][0]:.2f}, "
            f"bwd-dz / fwd = {res['bwd-dz'][0] / res['fwd'][0]:.2f}; {100 * zero_share:.0f} % of the codes are 0; {rows} workgroups on 256 CUs")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
