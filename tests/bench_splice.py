"""The splice attack and the masked detection losses (a benchmark, not a test):
    python tests/bench_splice.py [--batch 256] [--rounds 7] [--out FILE] [--no-step] [--no-eval]
It times, alternating in the same process, at logits [2 * batch, 16000, 17] and signals [batch, 16000] fp32,
  bce_fwd / bce_masked_fwd   wm_bce_fwd against wm_bce_masked_fwd on the same logits (labels drawn by wm_splice);
  bce_bwd / bce_masked_bwd   the same for the gradient pass;
  splice / splice_bwd        wm_splice (default spans of attacks.Splice) and wm_splice_bwd;
  copy                       a device-to-device hipMemcpyAsync of one signal frame, the bytes a splice moves at least;
each as the median over `--rounds` rounds of a batch of launches sized to at least `--batch-seconds` of device time between two events
(after a warm-up), the spread being (max - min) / median over the rounds, and max / min over the rounds of the unmasked kernels, the
yardstick the masked ones are held against.  Then, unless switched off, the train step (FlatAdam, bench.py's synthetic batch) with and
without tamper=Splice() in alternation, and evaluate_localization of the golden Detector checkpoint behind an untrained Generator."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import awm_amd                                                        # noqa: E402
from awm_amd.ops import _stream                                       # noqa: E402
from bench_timing import batch_ms, launches_for                       # noqa: E402

T, NO = 16000, 17


def stats(v):
    v = sorted(v)
    med = v[len(v) // 2]
    return med, (v[-1] - v[0]) / med, v[-1] / v[0]


def device_copy(dst, src):
    """hipMemcpyAsync, device to device, on the current stream (Tensor.copy_ where the runtime library cannot be opened by name)"""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        fn = hip.hipMemcpyAsync
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        fn.restype = ctypes.c_int
        nbytes = src.numel() * src.element_size()
        return (lambda: fn(dst.data_ptr(), src.data_ptr(), nbytes, 3, _stream())), "hipMemcpyAsync"
    except (OSError, AttributeError):
        return (lambda: dst.copy_(src, non_blocking=True)), "Tensor.copy_"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-eval", action="store_true")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_splice.py measures on the GPU"
    lib = awm_amd.lib
    lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, R = a.batch, 2 * a.batch
    gen = torch.Generator(device=dev).manual_seed(1)
    tamper = awm_amd.Splice(seed=1234)
    cut = tamper.cut(T)
    x = torch.randn(B, T, device=dev, generator=gen) * 0.3
    clean = torch.randn(B, T, device=dev, generator=gen) * 0.3
    out = torch.empty_like(x)
    W = (T + 31) // 32
    lab = torch.empty(B, W, dtype=torch.int32, device=dev)
    ones = torch.full((B, W), -1, dtype=torch.int32, device=dev)
    logits = torch.randn(R, T, NO, device=dev, generator=gen) * 3.0
    dlogits = torch.empty_like(logits)
    msg = torch.randint(0, 2 ** 16, (B,), device=dev, generator=gen)
    part = torch.empty(3 * R * ((T * NO + 4095) // 4096), device=dev)
    res2, count = torch.zeros(2, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    g = torch.ones(1, device=dev)
    P = lambda t: t.data_ptr()                                        # noqa: E731

    def splice():
        lib.wm_splice(P(x), P(clean), P(out), P(lab), B, T, 0, 1234, 0, cut["max_spans"], cut["p_span"], cut["len_lo"], cut["len_hi"],
                      cut["p_original"], cut["p_silence"], _stream())
    splice()
    copy, copy_name = device_copy(out, x)
    frac = float(torch.from_numpy(awm_amd.unpack_labels(lab, T)).float().mean())
    codes = {
        "bce_fwd": lambda: lib.wm_bce_fwd(P(logits), P(msg), P(part), P(res2[0]), P(res2[1]), B, R, T, NO, _stream()),
        "bce_masked_fwd": lambda: lib.wm_bce_masked_fwd(P(logits), P(msg), P(lab), P(part), P(count), P(res2[0]), P(res2[1]), B, R, T, NO, _stream()),
        "bce_bwd": lambda: lib.wm_bce_bwd(P(logits), P(msg), P(g), P(g), P(dlogits), B, R, T, NO, _stream()),
        "bce_masked_bwd": lambda: lib.wm_bce_masked_bwd(P(logits), P(msg), P(lab), P(count), P(g), P(g), P(dlogits), B, R, T, NO, _stream()),
        "splice": splice,
        "splice_bwd": lambda: lib.wm_splice_bwd(P(x), P(lab), P(out), B, T, _stream()),
        "copy": copy,
    }
    lbytes, sbytes = R * T * NO * 4, B * T * 4
    nbytes = {"bce_fwd": lbytes, "bce_masked_fwd": lbytes + B * W * 8, "bce_bwd": 2 * lbytes, "bce_masked_bwd": 2 * lbytes + B * W * 4,
              "splice": 2 * sbytes + B * W * 4, "splice_bwd": 2 * sbytes + B * W * 4, "copy": 2 * sbytes}
    say(f"# B = {B}, T = {T}, NO = {NO}; median of {a.rounds} rounds, each >= {a.batch_seconds} s of launches; spread = (max - min) / median; "
        f"copy = {copy_name}; labels: {100 * frac:.1f}% of the samples still watermarked")
    say(f"{'code':>16} {'us':>9} {'spread':>7} {'max/min':>8} {'MB':>8} {'GB/s':>7} {'launches':>8}")
    k = {c: launches_for(fn, a.batch_seconds, 20000) for c, fn in codes.items()}
    times = {c: [] for c in codes}
    for _ in range(a.rounds):                                         # alternate the codes inside every round
        for c, fn in codes.items():
            times[c].append(batch_ms(fn, k[c]))
    res = {c: stats(v) for c, v in times.items()}
    for c in codes:
        med, spread, ratio = res[c]
        mb = nbytes[c] / 1e6
        say(f"{c:>16} {1e3 * med:9.2f} {100 * spread:6.1f}% {ratio:8.3f} {mb:8.2f} {mb / med:7.0f} {k[c]:8d}")
    for masked, plain in (("bce_masked_fwd", "bce_fwd"), ("bce_masked_bwd", "bce_bwd")):
        say(f"# {masked} / {plain} = {res[masked][0] / res[plain][0]:.3f}; max / min over the repeats of {plain} alone = {res[plain][2]:.3f}")
    say(f"# splice / copy = {res['splice'][0] / res['copy'][0]:.2f}, splice_bwd / copy = {res['splice_bwd'][0] / res['copy'][0]:.2f}")
    # the same with every label 1: the masked kernels read the mask, whatever it holds
    lib.wm_bce_masked_fwd(P(logits), P(msg), P(ones), P(part), P(count), P(res2[0]), P(res2[1]), B, R, T, NO, _stream())
    torch.cuda.synchronize()
    assert int(count) == B * T
    del logits, dlogits

    if not a.no_step:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        torch.manual_seed(42)
        G, D = awm_amd.Generator(16).to(dev).train(), awm_amd.Detector(16).to(dev).train()
        opt = awm_amd.FlatAdam([G, D], lr=1e-3)
        gs = torch.Generator().manual_seed(1234)
        s = (0.1 * torch.randn(B, 1, T, generator=gs)).clamp_(-0.99, 0.99).to(dev)
        m = torch.randint(0, 2 ** 16, (B,), generator=torch.Generator().manual_seed(4321)).to(dev)
        steps = {"plain": lambda: awm_amd.train_step(G, D, opt, s, m), "tamper": lambda: awm_amd.train_step(G, D, opt, s, m, tamper=tamper)}
        for fn in steps.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        st = {c: [] for c in steps}
        for _ in range(a.step_rounds):
            for c, fn in steps.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                st[c].append((time.perf_counter() - t0) / 3 * 1e3)
        sres = {c: stats(v) for c, v in st.items()}
        for c in steps:
            say(f"# train step B = {B}, {c:>6}: {sres[c][0]:8.2f} ms (median of {a.step_rounds} x 3 steps, max / min {sres[c][2]:.3f})")
        say(f"# train step tamper / plain = {sres['tamper'][0] / sres['plain'][0]:.3f} (the unfused Detector tail, wm_splice, the masked losses)")
        del G, D, opt

    if not a.no_eval:
        from oracle import wm_oracle as O
        ck = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detector_best_unprefixed.npz"))
        D = awm_amd.Detector(16)
        D.load_state_dict({key: torch.from_numpy(ck[key]) for key in ck.files})
        torch.manual_seed(17)
        G = awm_amd.Generator(16)
        G.to(dev); D.to(dev)
        batches = [O.synthetic_clips(8, seed=51 + i) for i in range(2)]
        messages = [O.synthetic_messages(8, seed=71 + i) for i in range(2)]
        row = awm_amd.evaluate_localization(G, D, batches, awm_amd.Splice(seed=5), device=dev, messages=messages)
        say("# evaluate_localization, golden Detector checkpoint (never trained to localise) behind an UNTRAINED Generator (manual_seed 17), "
            "16 synthetic clips, Splice(seed=5) defaults:")
        say("# " + ", ".join(f"{key} = {v:.4f}" if isinstance(v, float) else f"{key} = {v}" for key, v in row.items()))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
