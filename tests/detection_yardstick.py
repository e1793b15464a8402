"""The yardsticks of the detection operating points: wm_clip_scores restated in float64 numpy (integers exact) with its case table,
input builder and tolerance floors, and a brute-force ROC -- a threshold loop over the distinct values and the O(n m) pair count.
For tests/test_detection_cpu.py and tests/test_gpu_clip_scores.py.  `import detection_yardstick as DY`.  Numpy and torch alone; nothing
from the package.

Floors of the rule max(8 * e32, floor) (loss_yardstick.held; the measure is max |a - ref| / max |ref|), from U = 2^-24 and the chunk
length kChunk = 8192 elements of csrc/clip_scores.hip.  The kernel's fp32 arithmetic ends at the chunk; the finish is fp64.
  llr.  Inside a chunk an element of channel o goes through one thread's chain and then the owner's four chains.  The thread stride is
      S = NO floor(256 / NO) >= 208 for NO in 1..64 (the minimum is at NO = 52), so a thread's chain has at most ceil(8192 / 208) = 40
      additions; the owner adds at most 256 thread sums in four chains of at most 64, and the chains in 2 more: an element meets at most
      40 + 64 + 2 = 106 roundings, one more for the final cast to fp32.  By the standard bound the sum's error is at most
      107 U sum |x|, so a mean's at most 107 U mean|x|: LLR_ROUNDINGS * U * (the largest channel mean of |x|) / (the largest |llr|).
      It depends on the case's data (through the float64 reference alone), because a mean of zero-mean logits is far smaller than the
      logits that were added.
  prob.  All terms are positive, so the bound is relative.  A chunk holds at most ceil(8192 / NO) channel-0 elements, 256 chains of at
      most 32, the 6 steps of the wave butterfly and 4 waves: 42 roundings.  The sigmoid 1 / (1 + expf(-x)): expf is within 1 ulp
      (2 U relative; the HIP math library's documented bound), which moves 1 / (1 + e) by at most 2 U relative, the addition and the
      IEEE division round once each: 4 U.  With the final cast: PROB_ROUNDINGS = 42 + 4 + 1 = 47, floor 47 U = 2.8e-6.
"""
import functools

import numpy as np
import torch

from yardstick_common import U

KCHUNK = 8192
LLR_ROUNDINGS = 107
PROB_ROUNDINGS = 47
PROB_FLOOR = PROB_ROUNDINGS * U

# (R, T, NO): one element; one sample of 17 channels; an odd T of two channels (a chunk boundary is never met); the widest NO at the
# wave size; 17 channels over 9 chunks with a ragged tail (4099 * 17 = 69683 = 8 * 8192 + 4147: an odd row length, so rows start at
# every alignment); 64 channels over 33 chunks, the stride S = 256; NO = 1 (every element is a sigmoid; S = 256); one long row of 5
# channels (43 chunks, S = 255); the clip of the flagship workload.  The CPU tests take the first five.
CASES = [(1, 1, 1), (3, 1, 17), (2, 63, 2), (2, 64, 64), (5, 4099, 17), (2, 4097, 64), (7, 1000, 1), (1, 70001, 5), (3, 16000, 17)]
CPU_CASES = CASES[:5]
THR_LOGITS = (0.0, 1.5, -np.inf, np.inf)
OFFSET = 0.05          # every channel's logits are shifted by +-OFFSET so that no mean sits at zero, where the soft bit would be a coin toss


def case_logits(R, T, NO):
    """float32 (R, T, NO): unit normal logits plus a per-(row, channel) offset of +-OFFSET, sign alternating.  soft_margin_ok holds for
    every case at these seeds; tests/test_detection_cpu.py asserts it."""
    g = torch.Generator().manual_seed(1000 * NO + T)
    x = torch.randn(R, T, NO, generator=g)
    sign = 1.0 - 2.0 * ((torch.arange(R)[:, None] + torch.arange(NO)[None, :]) % 2).float()
    return (x + OFFSET * sign[:, None, :]).contiguous()


def case_message(R, NO, B):
    g = torch.Generator().manual_seed(7 * NO + R)
    return torch.randint(0, 2 ** 62, (B,), generator=g, dtype=torch.int64) & ((1 << (NO - 1)) - 1)


def clip_scores_ref(logits, message=None, thr_logit=0.0):
    """wm_clip_scores in float64, channel by channel: {"prob" (R,), "llr" (R, NO), "total" (R, NO) float64; "votes" (R, NO) int32;
    "words" (R, 2) int64; "biterr" (B, 2) int32}.  thr_logit is rounded to float32 first, as the C ABI takes it."""
    x = np.asarray(logits, dtype=np.float64)
    R, T, NO = x.shape
    thr = float(np.float32(thr_logit))
    votes = np.zeros((R, NO), dtype=np.int32)
    total = np.zeros((R, NO))
    words = np.zeros((R, 2), dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        prob = np.array([np.sum(1.0 / (1.0 + np.exp(-x[r, :, 0]))) / T for r in range(R)])
        for r in range(R):
            hard = soft = 0
            for o in range(NO):
                col = x[r, :, o]
                votes[r, o] = int(np.count_nonzero(col > (thr if o == 0 else 0.0)))
                total[r, o] = np.sum(col)
                if o >= 1:
                    hard |= int(2 * int(votes[r, o]) > T) << (o - 1)
                    soft |= int(total[r, o] > 0.0) << (o - 1)
            words[r] = (hard, soft)
    B = 0 if message is None else len(message)
    biterr = np.zeros((B, 2), dtype=np.int32)
    for r in range(B):
        for k in range(2):
            biterr[r, k] = bin((int(words[r, k]) ^ int(message[r])) & ((1 << (NO - 1)) - 1)).count("1")
    return {"prob": prob, "llr": total / T, "total": total, "votes": votes, "words": words, "biterr": biterr}


def torch32(logits):
    """the float32 torch restatement on the CPU (step._eval_reductions' expressions): (prob, llr)"""
    x = torch.as_tensor(logits, dtype=torch.float32)
    return torch.sigmoid(x[:, :, 0]).mean(dim=1), x.mean(dim=1)


def llr_floor(logits):
    x = np.abs(np.asarray(logits, dtype=np.float64))
    return LLR_ROUNDINGS * U * float(x.mean(axis=1).max()) / float(np.abs(np.asarray(logits, dtype=np.float64).mean(axis=1)).max())


def rel_err(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max() / (np.abs(ref).max() + 1e-30))


@functools.lru_cache(maxsize=None)
def case(R, T, NO):
    """the case's logits, its float64 reference at thr_logit = 0 without a message, the float32 restatement and the two bars"""
    x = case_logits(R, T, NO)
    ref = clip_scores_ref(x.numpy())
    p32, l32 = torch32(x)
    bars = {"prob": max(8 * rel_err(p32.numpy(), ref["prob"]), PROB_FLOOR), "llr": max(8 * rel_err(l32.numpy(), ref["llr"]), llr_floor(x.numpy()))}
    return x, ref, (p32, l32), bars


def soft_margin_ok(R, T, NO):
    """every channel's |mean logit| exceeds the llr bar times max |logit|: an error inside the bar (which is relative to max |llr| <=
    max |logit|) cannot move a soft bit"""
    x, ref, _, bars = case(R, T, NO)
    return float(np.abs(ref["llr"]).min()) > bars["llr"] * float(x.abs().max())


# ------------------------------------------------------------------------------------------------------------ brute-force ROC
def roc_brute(clean, marked):
    """(thresholds, fp, tp): +inf and every distinct value descending; counts of scores >= threshold, one comparison loop per threshold"""
    clean, marked = [float(v) for v in clean], [float(v) for v in marked]
    thr = [float("inf")] + sorted(set(clean) | set(marked), reverse=True)
    return thr, [sum(1 for c in clean if c >= t) for t in thr], [sum(1 for m in marked if m >= t) for t in thr]


def auc_pairs(clean, marked):
    """2 #{(m, c): m > c} + #{(m, c): m == c} over all pairs, as a Python integer: the numerator of AUC over 2 n_clean n_marked"""
    clean, marked = [float(v) for v in clean], [float(v) for v in marked]
    return sum(2 * (m > c) + (m == c) for m in marked for c in clean)
