"""The clip-curation launches (a benchmark, not a test):
    python tests/bench_curate.py [--rounds 7] [--out FILE]
It times, alternating in the same process,
  feat     wm_clip_features alone on x (512, 16000) fp32 at 16 kHz, outputs allocated once: the one launch;
  ops      ops.clip_features on the same rows (the launch plus its three output allocations);
  frames   the same with the per-frame table written as well;
  mul      torch.mul(x, 0.7, out=out) over the same tensor: a plain pass, for scale;
then curate.prepare_recording on one ten-minute recording -- at 16 kHz mono (peak, scale, cut, one feature launch over 600 clips) and at
44.1 kHz stereo (the mix-down and resampling launch first);
each as the median over `--rounds` rounds of a batch of launches sized to at least `--batch-seconds` of device time between two events
(after a warm-up), the spread being (max - min) / median over the rounds.  The bytes the algorithm needs are the rows read once; they are
set against the 8 TB/s of the data sheet.  Against the launch, the host path (the float64 numpy restatement the package runs for CPU
tensors: what the reference's per-file librosa and scipy calls cost in kind, not librosa itself) on `--host-rows` of the same rows in
this one process, timed once with a host clock and scaled to 512 rows.  Before anything is timed the device features of those rows are
compared with the host's."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import awm_amd                                                        # noqa: E402
from awm_amd import curate, ops                                       # noqa: E402
from awm_amd.ops import _stream                                       # noqa: E402
from bench_timing import measure                                      # noqa: E402
import curate_yardstick as Y                                          # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--host-rows", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_curate.py measures on the GPU"
    lib = awm_amd.lib
    lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rows, n, sr = 512, 16000, 16000
    base = Y.make_rows(48, n, sr)
    x_host = torch.from_numpy(base[np.arange(rows) % 48].copy())
    x = x_host.to(dev)
    plan = ops.clip_features_plan(rows, n, sr)
    tab = curate.tables_on(sr, dev)
    nbytes = 4 * rows * n
    say(f"# x ({rows}, {n}) at {sr} Hz, {plan.frames} spectral frames a row, {plan.lds_bytes} bytes of LDS a workgroup, band-pass warm-up "
        f"{tab['warm']}; median of {a.rounds} rounds, each >= {a.batch_seconds} s of launches; spread = (max - min) / median")
    say(f"# bytes the launch needs: the rows once = {nbytes / 1e6:.1f} MB = {1e6 * nbytes / PEAK_BYTES_PER_S:.1f} us at 8 TB/s")
    feat, counts = ops.clip_features(x, sr)
    t0 = time.perf_counter()
    hf, hc = curate.clip_features_host(x_host[:a.host_rows].numpy(), sr)
    host_ms = (time.perf_counter() - t0) * 1e3 * rows / a.host_rows
    err = Y.rel_error(feat[:a.host_rows, :13].cpu().numpy(), hf[:, :13])
    same = bool((counts[:a.host_rows].cpu().numpy() == hc).all())
    say(f"# device against host on {a.host_rows} rows: largest relative distance {err.max():.2e} ({Y.FEATURES[int(err.argmax())]}), integers equal: {same}; "
        f"labels of the {rows} rows: {int((counts[:, 3] == 1).sum())} speech, {int((counts[:, 3] == 0).sum())} noise")
    assert err.max() < 1e-4 and same
    out = torch.empty_like(x)
    per = torch.empty(rows, plan.frames, 4, device=dev)
    ptr = [t.data_ptr() for t in (x, tab["sos"], tab["fb"], tab["klo"], tab["khi"], tab["dct"], feat, counts)]
    runs = {
        "feat": lambda: lib.wm_clip_features(*ptr, None, rows, n, sr, tab["warm"], _stream()),
        "ops": lambda: ops.clip_features(x, sr),
        "frames": lambda: lib.wm_clip_features(*ptr, per.data_ptr(), rows, n, sr, tab["warm"], _stream()),
        "mul": lambda: torch.mul(x, 0.7, out=out),
    }
    say(f"{'input':>22} {'code':>8} {'us':>10} {'spread':>7} {'GB/s':>8} {'of 8 TB/s':>9} {'x host':>8} {'launches':>8}")
    res = measure(runs, a.rounds, a.batch_seconds)
    for c, (med, spread, k) in res.items():
        rate = nbytes / (med * 1e-3) * (2 if c == "mul" else 1)
        ratio = f"{host_ms / med:8.0f}" if c != "mul" else ""
        say(f"{'(512, 16000)':>22} {c:>8} {1e3 * med:10.2f} {100 * spread:6.1f}% {rate / 1e9:8.0f} {100 * rate / PEAK_BYTES_PER_S:8.2f}% {ratio:>8} {k:8d}")
    say(f"# host path (float64 numpy, one process): {host_ms:.0f} ms for {rows} rows, scaled from {a.host_rows} rows")
    del runs, res
    # one ten-minute recording
    mono = x.reshape(-1).repeat(-(-9_600_000 // (rows * n)))[:9_600_000].reshape(1, -1).contiguous()
    t = torch.arange(int(600 * 44100), device=dev) / 44100.0
    stereo = torch.stack([0.3 * torch.sin(2 * np.pi * 170.0 * t) * (0.1 + torch.sin(2 * np.pi * 3.0 * t) ** 2),
                          0.02 * torch.randn(t.numel(), device=dev, generator=torch.Generator(device=dev).manual_seed(3))])
    del t
    clips, table = curate.prepare_recording(mono, 16000, device=dev)
    say(f"# ten minutes at 16 kHz mono: {clips.shape[0]} clips, {int((table['classification'] == 1).sum())} speech, {int(table['silent'].sum())} silent")
    clips, table = curate.prepare_recording(stereo, 44100, device=dev)
    say(f"# ten minutes at 44.1 kHz stereo: {clips.shape[0]} clips, {int((table['classification'] == 1).sum())} speech, {int(table['silent'].sum())} silent")
    res = measure({"prep16": lambda: curate.prepare_recording(mono, 16000, device=dev),
                   "prep44": lambda: curate.prepare_recording(stereo, 44100, device=dev)}, a.rounds, a.batch_seconds)
    for c, (med, spread, k) in res.items():
        src = mono if c == "prep16" else stereo
        say(f"{str(tuple(src.shape)):>22} {c:>8} {1e3 * med:10.2f} {100 * spread:6.1f}% {'':>8} {'':>9} {'':>8} {k:8d}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
