"""The noise-suppression launches (a benchmark, not a test):
    python tests/bench_noise_suppress.py [--rounds 7] [--out FILE]
It times, alternating in the same process, on x (512, 16000) fp32 at 16 kHz,
  fwd        wm_noise_suppress alone (three launches), buffers allocated once, no gains written: the evaluation number;
  fwd+gains  the same with gain_out and noise_out written;
  fwd+bwd    NoiseSuppress()(x).backward(dy) through autograd: what a train step pays, two calls and their allocations;
  torch fwd  the same definition in torch ops on the same GPU (torch.stft, the frame loop, torch.istft) under no_grad: the yardstick;
  torch f+b  that restatement with autograd through it, the gains detached: the thing the kernels stand in for;
  mul        torch.mul(x, 0.7, out=out) over one (512, 16000) tensor: a plain pass, for scale;
then one row of 57.6 M samples (an hour) through fwd; each as the median over `--rounds` rounds of a batch of launches sized to at least
`--batch-seconds` of device time between two events (after a warm-up), the spread being (max - min) / median over the rounds.  Against
them, the host path (the float64 numpy restatement CPU tensors take) on `--host-rows` of the same rows, timed once with a host clock and
scaled to 512 rows.  Before anything is timed the device's numbers are compared with the host's and with the torch restatement's."""
import argparse
import importlib
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import awm_amd                                                        # noqa: E402
from awm_amd.ops import _stream                                       # noqa: E402
from bench_timing import measure                                      # noqa: E402
import suppress_yardstick as Y                                        # noqa: E402

S = importlib.import_module("awm_amd.suppress")


def torch_model(x, reduce_db, window, alpha=0.98, over=1.0, src=None):
    """y (rows, n) in torch ops: the definition of include/wm_hip.h with torch.stft, a loop over the frames and torch.istft; the gains
    are detached, as the kernels hold them"""
    rows, n = x.shape
    M = -(-n // 256) + 1
    kw = dict(n_fft=512, hop_length=256, win_length=512, window=window, center=False)
    pad = lambda v: torch.nn.functional.pad(v, (256, (M + 1) * 256 - 256 - n))     # noqa: E731
    X = torch.stft(pad(x), return_complex=True, **kw)                              # (rows, 257, M)
    with torch.no_grad():
        P = X.real ** 2 + X.imag ** 2
        N = math.exp(Y.GAMMA_E) * torch.exp(torch.log(P + Y.EPS).mean(dim=2))
        g = P / (over * N + Y.EPS)[:, :, None]
        gmin = (10.0 ** (-reduce_db.clamp(0.0, 60.0) / 20.0))[:, None]
        q = torch.ones_like(N)
        G = []
        for m in range(M):
            xi = alpha * q + (1.0 - alpha) * (g[:, :, m] - 1.0).clamp(min=0.0)
            Gm = torch.maximum(xi / (1.0 + xi), gmin)
            q = Gm * Gm * g[:, :, m]
            G.append(Gm)
        G = torch.stack(G, dim=2)
    Sx = X if src is None else torch.stft(pad(src), return_complex=True, **kw)
    out = torch.istft(G * Sx, length=(M + 1) * 256, **kw)
    return out[:, 256:256 + n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--host-rows", type=int, default=8)
    ap.add_argument("--long-seconds", type=int, default=3600)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_noise_suppress.py measures on the GPU"
    lib = awm_amd.lib
    lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import numpy as np
    rows, n = 512, 16000
    rng = np.random.default_rng(5)
    x_host = torch.from_numpy(np.stack([Y.voiced(n, 900 + i) + 0.005 * rng.standard_normal(n) for i in range(rows)]).astype(np.float32))
    rd_host = torch.tensor([6.0 + 18.0 * (i % 7) / 6.0 for i in range(rows)])
    x, rd = x_host.to(dev), rd_host.to(dev)
    dy = torch.randn(rows, n, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    window = torch.from_numpy(Y.window()).to(torch.float32).to(dev)

    def buffers(r, m):
        frames, need = S.suppress_plan(r, m)
        return dict(y=torch.empty(r, m, device=dev), G=torch.empty(r, frames, 257, device=dev), N=torch.empty(r, 257, device=dev),
                    scratch=torch.empty(need // 4, dtype=torch.int32, device=dev), frames=frames, need=need)

    def call(xs, rds, b, gains):
        r, m = xs.shape
        return lambda: lib.wm_noise_suppress(xs.data_ptr(), None, None, rds.data_ptr(), b["y"].data_ptr(), b["G"].data_ptr() if gains else None,
                                             b["N"].data_ptr() if gains else None, b["scratch"].data_ptr(), r, m, 0.98, 1.0, _stream())

    b = buffers(rows, n)
    io = 2 * rows * n * 4
    pg = rows * b["frames"] * 257 * 4
    say(f"# x ({rows}, {n}) at 16 kHz, harmonic rows plus noise at RMS 0.005, reduce_db 6..24 by row; {b['frames']} frames a row; median of "
        f"{a.rounds} rounds, each >= {a.batch_seconds} s of launches; spread = (max - min) / median")
    say(f"# bytes: x in + y out = {io / 1e6:.1f} MB; scratch {b['need'] / 1e6:.1f} MB of which P / G {pg / 1e6:.1f} MB; a forward reads x twice, "
        f"writes and reads P, writes and reads G (twice) and writes y: {(3 * rows * n * 4 + 5 * pg) / 1e6:.0f} MB")
    # the numbers before they are timed
    call(x, rd, b, True)()
    with torch.no_grad():
        yt = torch_model(x, rd, window)
    t0 = time.perf_counter()
    hy, hG, hN = S.suppress_rows_host(x_host[:a.host_rows], rd_host[:a.host_rows], gains_out=True)
    host_ms = (time.perf_counter() - t0) * 1e3 * rows / a.host_rows
    hr = slice(0, a.host_rows)
    e_y = float(((b["y"][hr].cpu() - hy).norm(dim=1) / hy.norm(dim=1)).max())
    e_G = float((b["G"][hr].cpu() - hG).abs().max())
    e_N = float(((b["N"][hr].cpu() - hN).abs().amax(dim=1) / hN.amax(dim=1)).max())
    e_t = float(((yt - b["y"]).norm(dim=1) / b["y"].norm(dim=1)).max())
    kept = float((b["y"].norm(dim=1) / x.norm(dim=1)).mean())
    say(f"# device against host on {a.host_rows} rows: y rel L2 {e_y:.2e}, |G| {e_G:.2e}, |N| / max N {e_N:.2e}")
    say(f"# torch restatement against device on {rows} rows: y rel L2 {e_t:.2e}; mean |y| / |x| {kept:.4f}, mean gain {float(b['G'].mean()):.4f}")
    assert e_y < 1e-5 and e_G < 1e-5 and e_N < 1e-5 and e_t < 1e-3
    out = torch.empty_like(x)
    mod = awm_amd.NoiseSuppress((6, 24))

    def loss_step():
        xl = x.detach().requires_grad_(True)
        mod(xl).backward(dy)

    def torch_fwd():
        with torch.no_grad():
            torch_model(x, rd, window)

    def torch_fb():
        xl = x.detach().requires_grad_(True)
        torch_model(xl, rd, window).backward(dy)

    runs = {
        "fwd": call(x, rd, b, False),
        "fwd+gains": call(x, rd, b, True),
        "fwd+bwd": loss_step,
        "torch fwd": torch_fwd,
        "torch f+b": torch_fb,
        "mul": lambda: torch.mul(x, 0.7, out=out),
    }
    say(f"{'rows':>14} {'code':>10} {'us':>10} {'spread':>7} {'x host':>9} {'GB/s of 2 rows n 4':>19} {'launches':>8}")
    res = measure(runs, a.rounds, a.batch_seconds)
    for c, (med, spread, k) in res.items():
        ratio = f"{host_ms / med:9.0f}" if c == "fwd+gains" else ""
        say(f"{'(512, 16000)':>14} {c:>10} {1e3 * med:10.2f} {100 * spread:6.1f}% {ratio:>9} {io / med / 1e6:19.0f} {k:8d}")
    say(f"# host path (float64 numpy, one process): {host_ms:.0f} ms for {rows} rows, scaled from {a.host_rows} rows")
    say(f"# torch restatement / kernels: forward {res['torch fwd'][0] / res['fwd'][0]:.1f} x, forward + backward {res['torch f+b'][0] / res['fwd+bwd'][0]:.1f} x")
    say(f"# fwd moves {(3 * rows * n * 4 + 5 * pg) / res['fwd'][0] / 1e6:.0f} GB/s of its own traffic (8000 GB/s is the memory's rate)")
    del runs, res, yt
    # one long row
    nl = a.long_seconds * 16000
    xl = x.reshape(-1).repeat(-(-nl // (rows * n)))[:nl].reshape(1, nl).contiguous()
    bl = buffers(1, nl)
    rdl = torch.full((1,), 18.0, device=dev)
    call(xl, rdl, bl, True)()
    torch.cuda.synchronize()
    say(f"# long row: {bl['frames']} frames, scratch {bl['need'] / 1e6:.0f} MB, y finite: {bool(torch.isfinite(bl['y']).all())}, "
        f"|y| / |x| {float(bl['y'].norm() / xl.norm()):.4f}, mean gain {float(bl['G'].mean()):.4f}")
    res = measure({"fwd": call(xl, rdl, bl, False)}, a.rounds, a.batch_seconds)
    for c, (med, spread, k) in res.items():
        say(f"{f'(1, {nl})':>14} {c:>10} {1e3 * med:10.2f} {100 * spread:6.1f}% {'':>9} {2 * nl * 4 / med / 1e6:19.0f} {k:8d}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
