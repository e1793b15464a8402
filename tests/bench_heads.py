"""Detector head launches at every supported width class (a benchmark, not a test):
    python tests/bench_heads.py [--out FILE]
Times wm_headN_fwd / wm_headN_bwd for NO = 1 + message_bits in {1, 2, 9, 17, 25, 33, 48, 64} at R = 512 clips x
T = 16000 with device events, and one train step at B = 256 with message_bits = 8.  Algorithmic bytes per sample:
forward (64 + NO) * 4 (read the frame, write the logits), backward (128 + NO) * 4 (read the frame and the logit
gradient, write the frame gradient)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import awm_amd                                                        # noqa: E402
from awm_amd import ops                                               # noqa: E402
from awm_amd.ops import NCU, _f32, _p, _stream, lib                   # noqa: E402
from oracle import wm_oracle as O                                     # noqa: E402

WIDTHS = (1, 2, 9, 17, 25, 33, 48, 64)


def timed(fn, warmup=3, reps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_heads.py measures on the GPU"
    awm_amd.lib.load()
    dev = torch.device("cuda:0")
    R, T = a.clips, 16000
    torch.manual_seed(0)
    x = torch.randn(R, 64, T, device=dev)
    dx = torch.empty_like(x)
    st = _stream()
    lines = [f"# wm_headN_fwd / wm_headN_bwd, R = {R} clips x T = {T}, {a.reps} timed repeats after 3 warm-up calls",
             f"{'NO':>3} {'fwd ms':>8} {'fwd GB/s':>9} {'bwd ms':>8} {'bwd GB/s':>9}"]
    print(lines[0]); print(lines[1])
    rows = {}
    for NO in WIDTHS:
        w = torch.randn(NO, 64, 1, device=dev) * 0.1
        b = torch.randn(NO, device=dev) * 0.1
        y = _f32(R, T, NO, device=dev)
        g = torch.randn(R, T, NO, device=dev)
        part = _f32(NCU * (NO * 64 + NO), device=dev)
        dw, db = torch.empty_like(w), _f32(NO, device=dev)
        tf = timed(lambda: lib.wm_headN_fwd(_p(x), _p(w), _p(b), _p(y), R, T, NO, st), reps=a.reps)
        tb = timed(lambda: lib.wm_headN_bwd(_p(g), _p(x), _p(w), _p(dx), _p(part), _p(dw), _p(db), R, T, NO, 0, st), reps=a.reps)
        bf, bb = R * T * (64 + NO) * 4, R * T * (128 + NO) * 4
        rows[NO] = (bf / tf / 1e6, bb / tb / 1e6)
        ln = f"{NO:3d} {tf:8.3f} {rows[NO][0]:9.0f} {tb:8.3f} {rows[NO][1]:9.0f}"
        print(ln, flush=True); lines.append(ln)
        del y, g, part
    ref = rows[17]
    ln = "# ratio to NO=17 (fwd, bwd): " + ", ".join(f"{n}: {rows[n][0] / ref[0]:.2f} / {rows[n][1] / ref[1]:.2f}" for n in WIDTHS)
    print(ln); lines.append(ln)
    del x, dx
    torch.cuda.empty_cache()

    # one train step at B = 256, message_bits = 8
    B = 256
    G, D = awm_amd.Generator(8).to(dev), awm_amd.Detector(8).to(dev)
    G.train(); D.train()
    opt = awm_amd.FlatAdam([G, D], lr=1e-3)
    s = O.synthetic_clips(B, seed=123).to(dev)
    msg = O.synthetic_messages(B, seed=124, bits=8).to(dev)
    ms = timed(lambda: awm_amd.train_step(G, D, opt, s, msg), warmup=3, reps=10)
    ln = f"# train step B={B}, message_bits=8: {ms:.2f} ms/step (10 steps after 3 warm-up steps)"
    print(ln); lines.append(ln)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
