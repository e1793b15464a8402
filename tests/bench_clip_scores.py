"""The per-clip score launch against the torch reductions it stands in for (a benchmark, not a test):
    python tests/bench_clip_scores.py [--rounds 7] [--out FILE]
On Detector-shaped logits (512, 16000, 17) -- the evaluation batch B = 256, watermarked and clean halves -- and (128, 16000, 17) it
times, alternating in the same process,
  kernel   ops.clip_scores(logits, message): wm_clip_scores' two launches plus the wrapper's six allocations;
  launch   wm_clip_scores alone through the C ABI, outputs and scratch allocated once;
  torch    the expressions of step._eval_reductions on the same logits: sigmoid of channel 0 and its mean, sigmoid of the bit channels
           of the watermarked half, compare, cast, mean, compare, and the comparison with the message bits;
each as the median over `--rounds` rounds of a batch of launches sized to at least `--batch-seconds` of device time between two events
(after a warm-up), the spread being (max - min) / median over the rounds.  The kernel's bytes are the logits read once, R T NO 4; they
are quoted over its time as a share of the HBM peak (8.0 TB/s by the data sheet; a float4 copy measures 6.29 TB/s on this chip).  The
smaller tensor (139 MB) fits the 256 MB Infinity Cache, so its rate is not an HBM rate.  Before anything is timed the kernel's bit
accuracy is compared with the torch expressions'."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import awm_amd                                                        # noqa: E402
from awm_amd import ops                                               # noqa: E402
from awm_amd.ops import _stream                                       # noqa: E402
from awm_amd.step import _eval_reductions                             # noqa: E402
from bench_timing import measure                                      # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.15)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_clip_scores.py measures on the GPU"
    lib = awm_amd.lib
    lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# median of {a.rounds} rounds, each >= {a.batch_seconds} s of launches; spread = (max - min) / median; share = R T NO 4 bytes / time / 8.0 TB/s")
    say(f"{'logits':>18} {'code':>7} {'us':>10} {'spread':>7} {'GB/s':>8} {'share':>6} {'launches':>8}")
    for R, T, NO in ((512, 16000, 17), (128, 16000, 17)):
        B = R // 2
        g = torch.Generator(device=dev).manual_seed(R)
        logits = torch.randn(R, T, NO, device=dev, generator=g) * 2.0
        message = torch.randint(0, 2 ** (NO - 1), (B,), device=dev, generator=g)
        delta = torch.zeros(B, 1, 4, device=dev)
        cs = ops.clip_scores(logits, message)
        ref = _eval_reductions(logits, message, delta)
        acc = (NO - 1 - cs.biterr[:, 0]).float() / (NO - 1)
        perr = float((cs.prob - torch.cat([ref["prob_watermarked"], ref["prob_clean"]])).abs().max())
        say(f"# ({R}, {T}, {NO}): bit accuracy equal to the torch expressions': {bool(torch.equal(acc, ref['bit_accuracy']))}; max |prob - torch's| {perr:.2e}")
        assert perr < 1e-5
        prob, llr = torch.empty(R, device=dev), torch.empty(R, NO, device=dev)
        votes = torch.empty(R, NO, dtype=torch.int32, device=dev)
        words = torch.empty(R, 2, dtype=torch.int64, device=dev)
        biterr = torch.empty(B, 2, dtype=torch.int32, device=dev)
        scratch = torch.empty(ops.clip_scores_plan(R, T, NO) // 4, dtype=torch.int32, device=dev)
        ptr = [t.data_ptr() for t in (logits, message, prob, llr, votes, words, biterr, scratch)]
        runs = {
            "kernel": lambda: ops.clip_scores(logits, message),
            "launch": lambda: lib.wm_clip_scores(ptr[0], ptr[1], 0.0, ptr[2], ptr[3], ptr[4], ptr[5], ptr[6], ptr[7], B, R, T, NO, _stream()),
            "torch": lambda: _eval_reductions(logits, message, delta),
        }
        res = measure(runs, a.rounds, a.batch_seconds)
        nbytes = R * T * NO * 4
        for c, (med, spread, k) in res.items():
            rate = nbytes / (med * 1e-3)
            share = f"{100 * rate / HBM_PEAK:5.1f}%" if c != "torch" else ""
            say(f"{str((R, T, NO)):>18} {c:>7} {1e3 * med:10.2f} {100 * spread:6.1f}% {rate / 1e9:8.0f} {share:>6} {k:8d}")
        say(f"# ({R}, {T}, {NO}): logits {nbytes / 1e6:.0f} MB, scratch {scratch.numel() * 4 / 1e6:.2f} MB; torch / kernel = {res['torch'][0] / res['kernel'][0]:.2f}")
        del runs, res, logits
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
