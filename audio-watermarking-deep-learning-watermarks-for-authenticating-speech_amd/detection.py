"""Detection operating points: ROC, AUC, EER, TPR at a set false-alarm rate, calibrated thresholds, message accuracy.

The reference pools one probability per clip and hands the pool to sklearn's roc_curve / auc / confusion_matrix / classification_report
(py/main16.py:2372-2386, the folder scans around :1575).  Here the per-clip numbers come from ONE wm_clip_scores launch per Detector
call (ops.clip_scores: the mean sigmoid, the mean logits, exact vote counts, the decoded words and their bit errors), and the curve is
a few lines of integer arithmetic on the pooled scores:

  host, pure numpy / Python integers    roc_curve, auc, auc_counts, eer, tpr_at_fpr, calibrate_threshold, operating_point,
                                        detection_report, clip_scores_host (the float64 restatement of wm_clip_scores)
  GPU loop                              evaluate_detection: attacks.evaluate_robustness's loop with operating points for rows

Two decision rules appear, as the two uses need them.  A ROC point is the rule "detected iff score >= threshold" at a threshold that IS
one of the scores (sklearn's convention); a calibrated or deployed threshold theta is the rule "detected iff score > theta" (the
reference's `probs > 0.5`), which is what calibrate_threshold and operating_point use.
"""
from __future__ import annotations

import math
from collections import OrderedDict, namedtuple

import numpy as np
import torch

RocCurve = namedtuple("RocCurve", "thresholds fp tp n_clean n_marked")
Calibration = namedtuple("Calibration", "threshold fpr n resolution")

SCORES = ("prob", "vote")
DECODES = ("vote", "llr")


def _scores(a, name):
    """a 1-D float64 array of finite scores (float32 values are carried exactly, so ties stay ties)"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    bad = int(np.count_nonzero(~np.isfinite(a)))
    if bad:
        raise ValueError(f"{name}: {bad} of {a.size} scores are not finite; a score that is NaN or infinite has no place on a ROC curve")
    return a


def _rate(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 1.0:      # NaN fails the comparison
        raise ValueError(f"{name}: expected a rate in [0, 1], got {v!r}")
    return float(v)


def _div(a, b):
    return a / b if b else math.nan


def roc_curve(clean_scores, marked_scores):
    """The whole ROC of "detected iff score >= threshold" in counts: RocCurve(thresholds, fp, tp, n_clean, n_marked).  thresholds: +inf,
    then every distinct score value of either class, descending; fp[i] / tp[i]: how many clean / marked scores are >= thresholds[i], as
    int64.  Every point is kept: sklearn.metrics.roc_curve(drop_intermediate=False) with fpr = fp / n_clean, tpr = tp / n_marked.
    Non-finite scores are refused (ValueError naming their number)."""
    clean, marked = np.sort(_scores(clean_scores, "clean_scores")), np.sort(_scores(marked_scores, "marked_scores"))
    thr = np.concatenate([[np.inf], np.unique(np.concatenate([clean, marked]))[::-1]])
    fp = (clean.size - np.searchsorted(clean, thr, side="left")).astype(np.int64)
    tp = (marked.size - np.searchsorted(marked, thr, side="left")).astype(np.int64)
    return RocCurve(thr, fp, tp, int(clean.size), int(marked.size))


def auc_counts(curve):
    """(numerator, denominator) of the trapezoid area as Python integers: sum_i (fp_i - fp_(i-1)) (tp_i + tp_(i-1)) and
    2 n_clean n_marked.  The numerator is the Mann-Whitney count 2 #{marked > clean} + #{marked == clean} over all pairs."""
    fp, tp = [int(v) for v in curve.fp], [int(v) for v in curve.tp]
    num = sum((fp[i] - fp[i - 1]) * (tp[i] + tp[i - 1]) for i in range(1, len(fp)))
    return num, 2 * curve.n_clean * curve.n_marked


def auc(curve):
    """The area under the curve, exact up to the one final division: the probability that a marked clip outscores a clean one, ties
    counting one half.  NaN when a class is empty."""
    num, den = auc_counts(curve)
    return _div(num, den)


def eer(curve):
    """The equal error rate: where FPR = 1 - TPR on the curve's polygon.  d_i = FPR_i - FNR_i rises strictly along the curve from -1 to
    +1 (every distinct threshold moves a count); at the first point with d_i >= 0 the answer is FPR_i if d_i = 0 (the tie rule: an
    exact crossing at a curve point is that point), else the linear interpolation between that point and the one before it, which is
    then the common value of FPR and FNR on the segment.  NaN when a class is empty."""
    nc, nm = curve.n_clean, curve.n_marked
    if nc == 0 or nm == 0:
        return math.nan
    d = [int(f) * nm - (nm - int(t)) * nc for f, t in zip(curve.fp, curve.tp)]              # (FPR - FNR) * nc * nm, exact
    i = next(k for k, v in enumerate(d) if v >= 0)                                          # d[-1] = nc * nm > 0; d[0] = -nc * nm < 0
    if d[i] == 0:
        return int(curve.fp[i]) / nc
    w = -d[i - 1] / (d[i] - d[i - 1])
    f0, f1 = int(curve.fp[i - 1]) / nc, int(curve.fp[i]) / nc
    return f0 + w * (f1 - f0)


def tpr_at_fpr(curve, target):
    """(tpr, threshold): the largest TPR among the curve's thresholds whose FPR <= target, and that threshold.  No interpolation: the
    pair is an operating point that "detected iff score >= threshold" achieves on these very clips (threshold +inf, TPR 0, when even
    the top clean score is too many).  (nan, nan) when a class is empty."""
    target = _rate(target, "target")
    if curve.n_clean == 0 or curve.n_marked == 0:
        return math.nan, math.nan
    ok = np.nonzero(curve.fp / curve.n_clean <= target)[0]                                  # fp rises with i, and so does tp
    i = int(ok[-1])
    return int(curve.tp[i]) / curve.n_marked, float(curve.thresholds[i])


def calibrate_threshold(clean_scores, target_fpr):
    """The threshold a deployment would fix in advance from clean audio alone: Calibration(threshold, fpr, n, resolution).  With
    k = floor(target_fpr * n), threshold is the smallest theta of the rule "detected iff score > theta" that lets at most k of the n
    clean scores through -- the (k + 1)-th largest clean score, or -inf if k >= n.  fpr is the rate observed at theta (ties can make it
    smaller than k / n), resolution = 1 / n the smallest rate n clips can resolve.
    A target below 1 / n gives k = 0: it is met by ZERO observed false alarms among n clips, which is not evidence of that rate --
    compare target_fpr with `resolution` before quoting it."""
    target = _rate(target_fpr, "target_fpr")
    clean = np.sort(_scores(clean_scores, "clean_scores"))[::-1]
    n = int(clean.size)
    if n == 0:
        raise ValueError("clean_scores: calibration needs at least one clean score")
    k = int(math.floor(target * n))
    theta = -math.inf if k >= n else float(clean[k])
    return Calibration(theta, int(np.count_nonzero(clean > theta)) / n, n, 1.0 / n)


def operating_point(clean_scores, marked_scores, threshold):
    """The confusion matrix of "detected iff score > threshold" and what a classification report derives from it, as numbers:
    {"tp", "fp", "fn", "tn", "precision", "recall", "f1", "accuracy"} (a ratio with an empty denominator is NaN)."""
    clean, marked = _scores(clean_scores, "clean_scores"), _scores(marked_scores, "marked_scores")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or math.isnan(threshold):
        raise ValueError(f"threshold: expected a number, got {threshold!r}")
    tp, fp = int(np.count_nonzero(marked > threshold)), int(np.count_nonzero(clean > threshold))
    fn, tn = int(marked.size) - tp, int(clean.size) - fp
    precision, recall = _div(tp, tp + fp), _div(tp, tp + fn)
    return OrderedDict(tp=tp, fp=fp, fn=fn, tn=tn, precision=precision, recall=recall, f1=_div(2 * tp, 2 * tp + fp + fn),
                       accuracy=_div(tp + tn, tp + fp + fn + tn))


def detection_report(marked, clean, biterr, bits, fpr_targets=(0.01,), threshold=0.5, deployed=None):
    """One row of evaluate_detection's table from pooled per-clip arrays: `marked` / `clean` the scores of the watermarked / clean
    clips, `biterr` the wrong bits per watermarked clip (ints; ignored when bits = 0), `bits` the message length.
    `deployed`: {target: theta} fixed in advance (evaluate_detection passes the thresholds calibrated on its "none" row's clean scores);
    None calibrates on this row's own `clean`.  Keys:
      auc, eer                 of the curve of marked against clean
      tpr_at_fpr               {target: (tpr, threshold)}: the best this row's own curve offers at FPR <= target
      deployed                 {target: (tpr, fpr)} of "score > theta" at the deployed theta: what a fixed threshold sees under the attack
      operating_point          operating_point(clean, marked, threshold)
      ber, message_accuracy    wrong bits / all bits, and the share of clips with EVERY bit right (NaN for bits = 0)
      clips, scores, curve     the number of marked clips, {"marked", "clean"} (the arrays as given) and the RocCurve"""
    targets = [_rate(t, "fpr_targets") for t in fpr_targets]
    curve = roc_curve(clean, marked)
    if deployed is None:
        deployed = {t: calibrate_threshold(clean, t).threshold for t in targets} if curve.n_clean else {}
    dep = OrderedDict()
    for t in targets:
        if t in deployed:
            op = operating_point(clean, marked, float(deployed[t]))
            dep[t] = (_div(op["tp"], curve.n_marked), _div(op["fp"], curve.n_clean))
    if bits > 0 and curve.n_marked > 0:
        be = np.asarray(biterr).reshape(-1).astype(np.int64)
        if be.size != curve.n_marked:
            raise ValueError(f"biterr: expected one count per marked clip ({curve.n_marked}), got {be.size}")
        ber, macc = int(be.sum()) / (be.size * bits), int(np.count_nonzero(be == 0)) / be.size
    else:
        ber, macc = math.nan, math.nan
    return OrderedDict(auc=auc(curve), eer=eer(curve), tpr_at_fpr=OrderedDict((t, tpr_at_fpr(curve, t)) for t in targets), deployed=dep,
                       operating_point=operating_point(clean, marked, threshold), ber=ber, message_accuracy=macc, clips=curve.n_marked,
                       scores={"marked": np.asarray(marked), "clean": np.asarray(clean)}, curve=curve)


def clip_scores_host(logits, message=None, thr_logit=0.0):
    """wm_clip_scores restated in float64 numpy (include/wm_hip.h has the definition): (prob, llr, votes, words, biterr) as arrays --
    prob (R,) and llr (R, NO) float64 (not yet rounded), votes (R, NO) int32, words (R, 2) int64, biterr (B, 2) int32 with B =
    len(message) or 0.  The integers are exact; the soft word tests the float64 sum."""
    x = np.asarray(logits)
    if x.ndim != 3 or min(x.shape) < 1:
        raise ValueError(f"logits: expected (R, T, NO) with every extent at least 1, got shape {x.shape}")
    x = x.astype(np.float64)
    R, T, NO = x.shape
    if NO > 64:
        raise ValueError(f"logits: at most 64 channels, got {NO}")
    thr = np.zeros(NO)
    thr[0] = float(np.float32(thr_logit))
    with np.errstate(over="ignore", invalid="ignore"):
        prob = (1.0 / (1.0 + np.exp(-x[:, :, 0]))).sum(axis=1) / T
        total = x.sum(axis=1)
    votes = (x > thr).sum(axis=1).astype(np.int32)                                          # NaN > anything is False
    weight = (1 << np.arange(NO - 1, dtype=np.int64))
    words = np.stack([((2 * votes[:, 1:].astype(np.int64) > T) * weight).sum(axis=1), ((total[:, 1:] > 0) * weight).sum(axis=1)],
                     axis=1).astype(np.int64)
    if message is None:
        biterr = np.zeros((0, 2), dtype=np.int32)
    else:
        msg = np.asarray(message, dtype=np.int64).reshape(-1)
        if msg.size > R:
            raise ValueError(f"message: at most one per row ({R}), got {msg.size}")
        diff = (words[:msg.size] ^ msg[:, None]) & np.int64((1 << (NO - 1)) - 1)
        biterr = np.array([[bin(int(v)).count("1") for v in row] for row in diff], dtype=np.int32).reshape(msg.size, 2)
    return prob, total / T, votes, words, biterr


@torch.no_grad()
def evaluate_detection(generator, detector, batches, attacks=None, device="cuda", message_bits=16, messages=None, fpr_targets=(0.01,),
                       threshold=0.5, score="prob", decode="vote", by_class=False):
    """Detection operating points under attacks: {"none": row, name: row, ...}, every row a detection_report.
    The loop is attacks.evaluate_robustness's -- eval mode, no_grad, the Generator once per batch, every attack applied to the
    concatenation of s + delta and s, the Detector once per attack -- with ONE ops.clip_scores call per Detector call in place of the
    torch reductions; the per-clip tensors stay on the device and are pooled once at the end.
      score   "prob": the clip's score is the mean sigmoid of channel 0 (the reference's);  "vote": the share of samples whose
              probability exceeds `threshold`, votes[:, 0] / T
      decode  "vote": the message is the majority of the per-sample hard decisions (the reference's);  "llr": the sign of the summed
              logits, words[:, 1]
    `threshold` is the probability both the per-sample vote and the row's "operating_point" use.  "tpr_at_fpr" is read off the row's own
    curve, i.e. calibrated on this attack's clean half; "deployed" applies the thresholds calibrated on the "none" row's clean scores
    under the attack.  message_bits = 0 gives NaN for "ber" and "message_accuracy".  `messages` (optional list, one tensor per batch)
    replaces the random draw.
    `by_class=True` adds "by_class" to every row: {"speech" | "noise" | "silent": a detection_report over that class's clips alone} (its
    "clips" is the class's count; "deployed" uses the thresholds calibrated on ALL clean clips of the "none" row), the classes being
    curate.clip_classes of the clean batch (one wm_clip_features launch per batch; a clip with a non-finite sample is in none)."""
    from . import dsp
    from .losses import postprocess
    if score not in SCORES:
        raise ValueError(f"score: expected one of {SCORES}, got {score!r}")
    if decode not in DECODES:
        raise ValueError(f"decode: expected one of {DECODES}, got {decode!r}")
    targets = [_rate(t, "fpr_targets") for t in fpr_targets]
    dsp.loc_threshold_logit(threshold)
    attacks = {} if attacks is None else attacks
    if "none" in attacks:
        raise ValueError('attacks: the name "none" is taken by the undistorted row')
    generator.eval(); detector.eval()
    named = [("none", None)] + list(attacks.items())
    acc = OrderedDict((name, ([], [], [])) for name, _ in named)                            # marked scores, clean scores, bit errors
    classes = []
    for bi, s in enumerate(batches):
        s = s.to(device)
        B = s.shape[0]
        if by_class:
            from .curate import clip_classes
            classes.append(clip_classes(s, 16000))
        message = (messages[bi].to(device) if messages is not None else
                   torch.randint(0, 2 ** message_bits, (B,), device=device))
        delta = postprocess(generator(s, message))
        both = torch.cat([s + delta, s], dim=0)
        for name, attack in named:
            logits = detector(both if attack is None else attack(both))
            cs = dsp.clip_scores(logits, message, threshold)
            sc = cs.prob if score == "prob" else cs.votes[:, 0].double() / logits.shape[1]
            acc[name][0].append(sc[:B])
            acc[name][1].append(sc[B:])
            acc[name][2].append(cs.biterr[:, 0 if decode == "vote" else 1])
    pooled = OrderedDict((name, [torch.cat(v).cpu().numpy() if v else np.zeros(0) for v in a]) for name, a in acc.items())
    clean0 = pooled["none"][1]
    deployed = {t: calibrate_threshold(clean0, t).threshold for t in targets} if clean0.size else {}
    res = OrderedDict((name, detection_report(m, c, be, message_bits, targets, threshold, deployed)) for name, (m, c, be) in pooled.items())
    if by_class:
        from .curate import CLASSES
        cls = torch.cat(classes).cpu().numpy() if classes else np.zeros(0, dtype=np.int64)
        for name, (m, c, be) in pooled.items():
            res[name]["by_class"] = OrderedDict((cname, detection_report(m[cls == i], c[cls == i], be[cls == i], message_bits, targets, threshold,
                                                                         deployed)) for i, cname in enumerate(CLASSES))
    return res
