"""The masking launches (a benchmark, not a test):
    python tests/bench_masking.py [--rounds 7] [--out FILE]
It times, alternating in the same process, on x, y (512, 16000) fp32 at 16 kHz,
  fwd        wm_masking_fwd alone (two launches), no coefficients kept: the evaluation number;
  fwd+coef   the same with the per-cell coefficients written: the forward of the loss;
  fwd+bwd    fwd+coef and wm_masking_bwd: the loss and its gradient, buffers allocated once;
  loss       MaskingLoss()(x, y).backward() through autograd: what a train step pays, allocations included;
  torch fwd  the same model in torch ops on the same GPU (torch.stft, matmuls for the bands and the spreading) under no_grad;
  torch f+b  that restatement with autograd through it, the mask detached: the thing the kernels stand in for;
  mul        torch.mul(x, 0.7, out=out) over one (512, 16000) tensor: a plain pass, for scale;
then one row of 57.6 M samples (an hour) through fwd and fwd+bwd; each as the median over `--rounds` rounds of a batch of launches sized
to at least `--batch-seconds` of device time between two events (after a warm-up), the spread being (max - min) / median over the rounds.
Against them, the host path (the float64 numpy restatement CPU tensors take) on `--host-rows` of the same rows, timed once with a host
clock and scaled to 512 rows.  Before anything is timed the device's numbers are compared with the host's and with the torch restatement's."""
import argparse
import importlib
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import awm_amd                                                        # noqa: E402
from awm_amd.ops import _stream                                       # noqa: E402
from bench_timing import measure                                      # noqa: E402
import masking_yardstick as Y                                         # noqa: E402

M = importlib.import_module("awm_amd.masking")


def torch_model(x, y, tab):
    """(nmr_db, over_db) per row in torch ops: the definition of include/wm_hip.h with torch.stft and matmuls, the mask detached"""
    kw = dict(n_fft=512, hop_length=256, win_length=512, window=tab["w"], center=False, return_complex=True)
    X, D = torch.stft(x, **kw), torch.stft(y - x, **kw)                                  # (rows, 257, F)
    c = tab["c"][None, :, None]
    Px, Pd = c * (X.real ** 2 + X.imag ** 2), c * (D.real ** 2 + D.imag ** 2)
    Ex, Ed = tab["onehot"] @ Px, tab["onehot"] @ Pd                                      # (rows, 22, F)
    inner = Px[:, 1:256]
    sfm = 10.0 * torch.log10(torch.exp(torch.log(inner + 1e-30).mean(dim=1)) / (inner.mean(dim=1) + 1e-30))
    alpha = (sfm / -60.0).clamp(0.0, 1.0)[:, None, :]
    O = alpha * (14.5 + tab["b"])[None, :, None] + (1.0 - alpha) * 5.5
    T = torch.maximum((tab["S"] @ Ex) * 10.0 ** (-O / 10.0) / tab["G"][None, :, None], tab["A"][None, :, None]).detach()
    r = Ed / T
    return 10.0 * torch.log10(r.mean(dim=(1, 2))), (10.0 * torch.log10(r.clamp(min=1.0))).mean(dim=(1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--host-rows", type=int, default=8)
    ap.add_argument("--long-seconds", type=int, default=3600)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_masking.py measures on the GPU"
    lib = awm_amd.lib
    lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import numpy as np
    rows, n = 512, 16000
    x_host = torch.from_numpy(np.stack([Y.voiced(n, 900 + i) for i in range(rows)]))
    level = torch.tensor([Y.LEVELS[i % 3] for i in range(rows)])[:, None]
    y_host = x_host + level * torch.randn(rows, n, generator=torch.Generator().manual_seed(2))
    x, y = x_host.to(dev), y_host.to(dev)
    host_tab = M.masking_tables()
    tab = {k: v.to(dev) for k, v in host_tab.items()}
    tab["onehot"] = torch.nn.functional.one_hot(tab["band"].long(), 22).T.float().contiguous()
    tab["b"] = torch.arange(22, device=dev, dtype=torch.float32)

    def buffers(r, m):
        frames, chunk, need = M.masking_plan(r, m)
        return dict(nmr=torch.empty(r, device=dev), over=torch.empty(r, device=dev), counts=torch.empty(r, 2, dtype=torch.int32, device=dev),
                    coef=torch.empty(r, frames, 22, device=dev), scratch=torch.empty(need // 4, dtype=torch.int32, device=dev),
                    gout=torch.full((r,), 1.0 / r, device=dev), gy=torch.empty(r, m, device=dev), frames=frames, chunk=chunk, need=need)

    def calls(xs, ys, b):
        r, m = xs.shape
        p = {k: v.data_ptr() for k, v in b.items() if isinstance(v, torch.Tensor)}
        px, py, pt = xs.data_ptr(), ys.data_ptr(), tab["packed"].data_ptr()
        fwd = lambda coef: lib.wm_masking_fwd(px, py, pt, p["nmr"], p["over"], p["counts"], coef, p["scratch"], r, m, _stream())   # noqa: E731
        bwd = lambda: lib.wm_masking_bwd(px, py, p["coef"], p["gout"], p["gy"], r, m, _stream())                                   # noqa: E731
        return fwd, bwd, p

    b = buffers(rows, n)
    fwd, bwd, p = calls(x, y, b)
    io = 2 * rows * n * 4
    say(f"# x, y ({rows}, {n}) at 16 kHz, delta at 1e-4 / 1e-3 / 1e-2 by row; {b['frames']} frames a row, {b['chunk']} a workgroup; median of {a.rounds} rounds, "
        f"each >= {a.batch_seconds} s of launches; spread = (max - min) / median")
    say(f"# bytes: inputs 2 * rows * n * 4 = {io / 1e6:.1f} MB; coef {b['coef'].numel() * 4 / 1e6:.2f} MB, scratch {b['need'] / 1e6:.3f} MB; "
        f"fwd moves inputs + coef = {(io + b['coef'].numel() * 4) / io:.2f} x the inputs, bwd inputs + coef + gy = {(1.5 * io + b['coef'].numel() * 4) / io:.2f} x")
    # the numbers before they are timed
    fwd(p["coef"]); bwd()
    yg = y.clone().requires_grad_(True)
    t_nmr, t_over = torch_model(x, yg, tab)
    t_over.mean().backward()
    t0 = time.perf_counter()
    hres, hgy = M.masking_rows_host(x_host[:a.host_rows], y_host[:a.host_rows], grad=True)
    host_ms = (time.perf_counter() - t0) * 1e3 * rows / a.host_rows
    hr = slice(0, a.host_rows)
    e_nmr = float((b["nmr"][hr].cpu() - hres.nmr_db).abs().max())
    e_over = float((b["over"][hr].cpu() - hres.over_db).abs().max())
    e_gy = float(((b["gy"][hr].cpu() * rows - hgy).norm(dim=1) / hgy.norm(dim=1).clamp(min=1e-30)).max())
    say(f"# device against host on {a.host_rows} rows: |nmr_db| {e_nmr:.2e} dB, |over_db| {e_over:.2e} dB, gradient rel L2 {e_gy:.2e}, "
        f"counts equal: {bool((b['counts'][hr, 0].cpu() == hres.audible).all())}")
    say(f"# torch restatement against device on {rows} rows: |nmr_db| {float((t_nmr.detach() - b['nmr']).abs().max()):.2e} dB, |over_db| "
        f"{float((t_over.detach() - b['over']).abs().max()):.2e} dB, gradient rel L2 {float((yg.grad - b['gy']).norm() / b['gy'].norm()):.2e}")
    say(f"# mean nmr_db {float(b['nmr'].mean()):.2f}, mean over_db {float(b['over'].mean()):.3f}, audible share "
        f"{float(b['counts'][:, 0].sum()) / float(b['counts'][:, 1].sum()):.3f}")
    assert e_nmr < 1e-4 and e_over < 1e-4 and e_gy < 1e-4
    out = torch.empty_like(x)
    loss_mod = awm_amd.MaskingLoss()

    def loss_step():
        yl = y.detach().requires_grad_(True)
        loss_mod(x, yl).backward()

    def torch_fwd():
        with torch.no_grad():
            torch_model(x, y, tab)

    def torch_fb():
        yl = y.detach().requires_grad_(True)
        torch_model(x, yl, tab)[1].mean().backward()

    runs = {
        "fwd": lambda: fwd(None),
        "fwd+coef": lambda: fwd(p["coef"]),
        "fwd+bwd": lambda: (fwd(p["coef"]), bwd()),
        "loss": loss_step,
        "torch fwd": torch_fwd,
        "torch f+b": torch_fb,
        "mul": lambda: torch.mul(x, 0.7, out=out),
    }
    say(f"{'rows':>14} {'code':>10} {'us':>10} {'spread':>7} {'x host':>9} {'GB/s of 2 rows n 4':>19} {'launches':>8}")
    res = measure(runs, a.rounds, a.batch_seconds)
    for c, (med, spread, k) in res.items():
        ratio = f"{host_ms / med:9.0f}" if c in ("fwd+bwd", "loss") else ""
        say(f"{'(512, 16000)':>14} {c:>10} {1e3 * med:10.2f} {100 * spread:6.1f}% {ratio:>9} {io / med / 1e6:19.0f} {k:8d}")
    say(f"# host path (float64 numpy with gradient, one process): {host_ms:.0f} ms for {rows} rows, scaled from {a.host_rows} rows")
    say(f"# torch restatement / kernels: forward {res['torch fwd'][0] / res['fwd'][0]:.1f} x, forward + backward {res['torch f+b'][0] / res['fwd+bwd'][0]:.1f} x")
    del runs, res, yg, t_nmr, t_over
    # one long row
    nl = a.long_seconds * 16000
    xl = x.reshape(-1).repeat(-(-nl // (rows * n)))[:nl].reshape(1, nl).contiguous()
    yl = xl + 1e-3 * torch.randn(1, nl, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    bl = buffers(1, nl)
    fwdl, bwdl, pl = calls(xl, yl, bl)
    fwdl(pl["coef"]); bwdl()
    torch.cuda.synchronize()
    say(f"# long row: {bl['frames']} frames, nmr_db {float(bl['nmr'][0]):.3f}, over_db {float(bl['over'][0]):.4f}, audible {int(bl['counts'][0, 0])} of "
        f"{int(bl['counts'][0, 1])} cells, gy finite: {bool(torch.isfinite(bl['gy']).all())}")
    res = measure({"fwd": lambda: fwdl(None), "fwd+bwd": lambda: (fwdl(pl["coef"]), bwdl())}, a.rounds, a.batch_seconds)
    for c, (med, spread, k) in res.items():
        say(f"{f'(1, {nl})':>14} {c:>10} {1e3 * med:10.2f} {100 * spread:6.1f}% {'':>9} {2 * nl * 4 / med / 1e6:19.0f} {k:8d}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
