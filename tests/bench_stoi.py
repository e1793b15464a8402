"""The STOI launches (a benchmark, not a test):
    python tests/bench_stoi.py [--rounds 7] [--out FILE]
It times, alternating in the same process,
  stoi16   ops.stoi on x, y (512, 16000) fp32 at 16 kHz: one resample_rows launch on the 1024 stacked rows, then wm_stoi's five launches;
  stoi10   wm_stoi alone on the same rows at 10 kHz (512, 10000), scratch allocated once;
  resamp   the resample_rows launch alone;
  mul      torch.mul(x, 0.7, out=out) over one (512, 16000) tensor: a plain pass, for scale;
then one row of 9.6 M samples at 16 kHz (ten minutes: 6 M samples and 46 873 frames at 10 kHz) through ops.stoi, and wm_stoi alone on it;
each as the median over `--rounds` rounds of a batch of launches sized to at least `--batch-seconds` of device time between two events
(after a warm-up), the spread being (max - min) / median over the rounds.  Against them, the host path (the float64 numpy restatement the
package runs for CPU tensors: what the reference's per-segment pystoi loop costs in kind, not pystoi itself) on `--host-rows` of the same
rows, timed once with a host clock and scaled to 512 rows, and on the first `--host-seconds` of the long row.  Before anything is timed the
device scores of those rows are compared with the host's."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import awm_amd                                                        # noqa: E402
from awm_amd import ops, quality                                      # noqa: E402
from awm_amd.ops import _stream                                       # noqa: E402
from bench_timing import measure                                      # noqa: E402
import stoi_yardstick as Y                                            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--host-rows", type=int, default=16)
    ap.add_argument("--host-seconds", type=int, default=60)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stoi.py measures on the GPU"
    lib = awm_amd.lib
    lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rows, n16 = 512, 16000
    import numpy as np
    x_host = torch.from_numpy(np.stack([Y.speech_like(n16, 900 + i) for i in range(rows)]))
    y_host = x_host + 0.03 * torch.randn(rows, n16, generator=torch.Generator().manual_seed(2))
    x, y = x_host.to(dev), y_host.to(dev)
    both = torch.cat([x, y])
    r10 = ops.resample_rows(both, 16000, 10000)
    x10, y10 = r10[:rows].contiguous(), r10[rows:].contiguous()
    n10 = x10.shape[1]
    d = torch.empty(rows, device=dev)
    kept = torch.empty(rows, dtype=torch.int32, device=dev)
    scratch = torch.empty(ops.stoi_plan(rows, n10) // 4, device=dev)
    out = torch.empty_like(x)
    say(f"# x, y ({rows}, {n16}) at 16 kHz -> ({rows}, {n10}) at 10 kHz; median of {a.rounds} rounds, each >= {a.batch_seconds} s of launches; spread = (max - min) / median")
    say(f"# scratch {scratch.numel() * 4 / 1e6:.2f} MB; bytes read by the five launches, counted: x, y twice = {4 * 4 * rows * n10 / 1e6:.1f} MB")
    # the scores before they are timed
    dd, kk = ops.stoi(x, y)
    t0 = time.perf_counter()
    hd, hk = quality.stoi_rows_host(x10[:a.host_rows].cpu(), y10[:a.host_rows].cpu())
    host_ms = (time.perf_counter() - t0) * 1e3 * rows / a.host_rows
    err = float((dd[:a.host_rows].cpu() - hd).abs().max())
    say(f"# device against host on {a.host_rows} rows: max |d - d_host| {err:.2e}, kept equal: {bool((kk[:a.host_rows].cpu() == hk).all())}, mean d {float(dd.mean()):.4f}")
    assert err < 1e-5
    px, py, pd, pk, ps = (t.data_ptr() for t in (x10, y10, d, kept, scratch))
    runs = {
        "stoi16": lambda: ops.stoi(x, y),
        "stoi10": lambda: lib.wm_stoi(px, py, pd, pk, ps, rows, n10, _stream()),
        "resamp": lambda: ops.resample_rows(both, 16000, 10000),
        "mul": lambda: torch.mul(x, 0.7, out=out),
    }
    say(f"{'rows':>14} {'code':>7} {'us':>10} {'spread':>7} {'x host':>9} {'launches':>8}")
    res = measure(runs, a.rounds, a.batch_seconds)
    for c, (med, spread, k) in res.items():
        ratio = f"{host_ms / med:9.0f}" if c.startswith("stoi") else ""
        say(f"{'(512, 16000)':>14} {c:>7} {1e3 * med:10.2f} {100 * spread:6.1f}% {ratio:>9} {k:8d}")
    say(f"# host path (float64 numpy, one process): {host_ms:.0f} ms for {rows} rows, scaled from {a.host_rows} rows")
    del runs, res
    # one long row
    nl = 9_600_000
    xl = x.reshape(-1).repeat(-(-nl // (rows * n16)))[:nl].reshape(1, nl).contiguous()
    yl = xl + 0.03 * torch.randn(1, nl, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    rl = ops.resample_rows(torch.cat([xl, yl]), 16000, 10000)
    xl10, yl10 = rl[:1].contiguous(), rl[1:].contiguous()
    nl10 = xl10.shape[1]
    dl = torch.empty(1, device=dev)
    kl = torch.empty(1, dtype=torch.int32, device=dev)
    sl = torch.empty(ops.stoi_plan(1, nl10) // 4, device=dev)
    dd, kk = ops.stoi(xl, yl)
    hn = a.host_seconds * 10000
    t0 = time.perf_counter()
    hd, hk = quality.stoi_rows_host(xl10[:, :hn].cpu(), yl10[:, :hn].cpu())
    host_long_ms = (time.perf_counter() - t0) * 1e3 * nl10 / hn
    dh, _ = ops.stoi(xl10[:, :hn].contiguous(), yl10[:, :hn].contiguous(), 10000)
    say(f"# long row: d {float(dd[0]):.4f}, kept {int(kk[0])} of {Y.frame_count(nl10)} frames; first {a.host_seconds} s device against host: |d - d_host| {abs(float(dh[0]) - float(hd[0])):.2e}")
    assert abs(float(dh[0]) - float(hd[0])) < 1e-5
    pxl, pyl, pdl, pkl, psl = (t.data_ptr() for t in (xl10, yl10, dl, kl, sl))
    res = measure({"stoi16": lambda: ops.stoi(xl, yl), "stoi10": lambda: lib.wm_stoi(pxl, pyl, pdl, pkl, psl, 1, nl10, _stream())},
                  a.rounds, a.batch_seconds)
    for c, (med, spread, k) in res.items():
        say(f"{'(1, 9600000)':>14} {c:>7} {1e3 * med:10.2f} {100 * spread:6.1f}% {host_long_ms / med:9.0f} {k:8d}")
    say(f"# host path on the long row: {host_long_ms:.0f} ms, scaled from its first {a.host_seconds} s")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
