"""Detection operating points without a GPU: the header and the exports, ops.clip_scores on CPU tensors against the float64 yardstick
and against step._eval_reductions' decoded bits, and the host functions of awm_amd.detection -- roc_curve / auc against a brute-force
threshold loop and pair count (and sklearn where it is installed), calibrate_threshold's defining inequality, a hand-built example
with its answers written out, detection_report on fabricated pools, and the argument checks."""
import math

import numpy as np
import pytest
import torch

import detection_yardstick as DY
from yardstick_common import ulp32


# ------------------------------------------------------------------------------------------------------------ header and exports
def test_the_header_declares_the_kernel_and_its_plan():
    from awm_amd import _lib
    protos = _lib.parse_header()
    assert [n for _, n in protos["wm_clip_scores_plan"]] == ["R", "T", "NO", "scratch_bytes", "stream"]
    assert [n for _, n in protos["wm_clip_scores"]] == ["logits", "message", "thr_logit", "prob", "llr", "votes", "words", "biterr", "scratch",
                                                        "B", "R", "T", "NO", "stream"]


def test_the_package_exports_the_new_names():
    import awm_amd
    for name in ("detection", "evaluate_detection", "detection_report", "roc_curve", "auc", "eer", "tpr_at_fpr", "calibrate_threshold",
                 "operating_point"):
        assert name in awm_amd.__all__ and hasattr(awm_amd, name), name
    assert callable(awm_amd.ops.clip_scores)


# ------------------------------------------------------------------------------------------------------------ ops.clip_scores on the CPU
@pytest.mark.parametrize("R,T,NO", DY.CASES)
def test_the_soft_bits_of_every_case_are_clear_of_the_bar(R, T, NO):
    assert DY.soft_margin_ok(R, T, NO), "choose another seed in detection_yardstick.case_logits"


def _clear_logits(R, T, NO):
    """the case's logits with every |l| either 0 or >= 1e-3, zeros of both signs planted, and (T even) one bit column of row 0 that is
    exactly half ones: a tie, so the bit is 0"""
    x = DY.case_logits(R, T, NO).clone()
    x[x.abs() < 1e-3] = 0.0
    flat = x.view(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    tie = None
    if T % 2 == 0 and NO > 1:
        tie = NO - 1
        x[0, :T // 2, tie] = 1.0
        x[0, T // 2:, tie] = -1.0
    return x, tie


@pytest.mark.parametrize("R,T,NO", DY.CPU_CASES)
@pytest.mark.parametrize("threshold", [0.5, 0.8])
def test_clip_scores_on_cpu_tensors_is_the_yardstick(R, T, NO, threshold):
    from awm_amd import ops
    x, tie = _clear_logits(R, T, NO)
    B = (R + 1) // 2
    msg = DY.case_message(R, NO, B)
    thr = ops.loc_threshold_logit(threshold)
    ref = DY.clip_scores_ref(x.numpy(), msg.numpy(), thr)
    got = ops.clip_scores(x, msg, threshold)
    assert got._fields == ("prob", "llr", "votes", "words", "biterr")
    assert (got.prob.dtype, got.llr.dtype, got.votes.dtype, got.words.dtype, got.biterr.dtype) == (
        torch.float32, torch.float32, torch.int32, torch.int64, torch.int32)
    assert tuple(got.biterr.shape) == (B, 2) and tuple(got.words.shape) == (R, 2)
    for k in ("votes", "words", "biterr"):
        assert np.array_equal(getattr(got, k).numpy(), ref[k]), k
    for k in ("prob", "llr"):
        r32 = ref[k].astype(np.float32).astype(np.float64)
        assert np.all(np.abs(getattr(got, k).numpy().astype(np.float64) - r32) <= 2 * ulp32(r32)), k
    if tie is not None:
        assert int(got.votes[0, tie]) * 2 == T and (int(got.words[0, 0]) >> (tie - 1)) & 1 == 0, "a tie decodes to 0"
    assert tuple(ops.clip_scores(x).biterr.shape) == (0, 2)
    if NO > 1:                                                         # the integer rule against the reference's float expressions
        from awm_amd.step import _eval_reductions
        out = _eval_reductions(x, msg, torch.zeros(B, 1, 4))
        bits = NO - 1
        assert torch.equal((bits - got.biterr[:, 0]).float() / bits, out["bit_accuracy"])


def test_clip_scores_checks_its_arguments():
    from awm_amd import ops
    x = torch.zeros(2, 3, 5)
    for bad in (x.double(), x[0], torch.zeros(2, 3, 65), torch.zeros(0, 3, 5)):
        with pytest.raises(ValueError):
            ops.clip_scores(bad)
    with pytest.raises(TypeError):
        ops.clip_scores(x.numpy())
    for msg in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int64)):
        with pytest.raises(ValueError):
            ops.clip_scores(x, msg)
    for thr in (-0.1, 1.5, math.nan, "0.5"):
        with pytest.raises(ValueError):
            ops.clip_scores(x, None, thr)
    with pytest.raises(ValueError):
        ops.clip_scores_plan(1, 2 ** 24 + 1, 1)


# ------------------------------------------------------------------------------------------------------------ ROC and AUC
def _beta_pool():
    rng = np.random.default_rng(5)
    clean = rng.beta(2.0, 5.0, 300).astype(np.float32)
    marked = rng.beta(5.0, 2.0, 200).astype(np.float32)
    marked[:20] = clean[:20]                                           # 20 forced cross-class ties
    return clean, marked


ROC_CASES = {
    "beta with ties": _beta_pool(),
    "all equal": (np.full(7, 0.25, np.float32), np.full(5, 0.25, np.float32)),
    "perfect": (np.linspace(0.0, 0.4, 9), np.linspace(0.6, 1.0, 6)),
    "inverted": (np.linspace(0.6, 1.0, 6), np.linspace(0.0, 0.4, 9)),
    "one clip per class": (np.array([0.2]), np.array([0.7])),
    "no marked clip": (np.array([0.2, 0.3]), np.zeros(0)),
    "no clean clip": (np.zeros(0), np.array([0.2, 0.3])),
}
ROC_AUC = {"all equal": 0.5, "perfect": 1.0, "inverted": 0.0, "one clip per class": 1.0}


@pytest.mark.parametrize("name", list(ROC_CASES))
def test_roc_and_auc_against_brute_force(name):
    from awm_amd import detection as D
    clean, marked = ROC_CASES[name]
    curve = D.roc_curve(clean, marked)
    thr, fp, tp = DY.roc_brute(clean, marked)
    assert curve.fp.dtype == np.int64 and curve.tp.dtype == np.int64
    assert list(curve.thresholds) == thr and [int(v) for v in curve.fp] == fp and [int(v) for v in curve.tp] == tp
    assert (curve.n_clean, curve.n_marked) == (len(clean), len(marked))
    num, den = D.auc_counts(curve)
    assert isinstance(num, int) and num == DY.auc_pairs(clean, marked) and den == 2 * len(clean) * len(marked)
    if den == 0:
        assert math.isnan(D.auc(curve)) and math.isnan(D.eer(curve)) and math.isnan(D.tpr_at_fpr(curve, 0.01)[0])
    else:
        assert D.auc(curve) == num / den
    if name in ROC_AUC:
        assert D.auc(curve) == ROC_AUC[name]


@pytest.mark.parametrize("name", [n for n, (c, m) in ROC_CASES.items() if len(c) and len(m)])
def test_roc_and_auc_against_sklearn(name):
    metrics = pytest.importorskip("sklearn.metrics")
    from awm_amd import detection as D
    clean, marked = ROC_CASES[name]
    curve = D.roc_curve(clean, marked)
    y = np.concatenate([np.zeros(len(clean)), np.ones(len(marked))])
    fpr, tpr, thr = metrics.roc_curve(y, np.concatenate([clean, marked]).astype(np.float64), drop_intermediate=False)
    assert np.array_equal(thr[1:], curve.thresholds[1:])               # (the first entry is +inf or max + 1, by sklearn version)
    assert np.allclose(fpr, curve.fp / curve.n_clean, rtol=0, atol=1e-12) and np.allclose(tpr, curve.tp / curve.n_marked, rtol=0, atol=1e-12)
    assert abs(metrics.auc(fpr, tpr) - D.auc(curve)) <= 1e-12


# ------------------------------------------------------------------------------------------------------------ calibration
def test_calibrate_threshold_is_the_smallest_threshold_within_the_budget():
    from awm_amd import detection as D
    rng = np.random.default_rng(9)
    clean = np.round(rng.beta(2.0, 5.0, 200), 2)                       # about 70 distinct values: ties everywhere
    n = clean.size
    distinct = np.unique(clean)
    for target in (0.0, 1.0 / n, 0.01, 0.5, 1.0):
        k = math.floor(target * n)
        cal = D.calibrate_threshold(clean, target)
        assert cal.n == n and cal.resolution == 1.0 / n
        above = int(np.count_nonzero(clean > cal.threshold))
        assert above <= k and cal.fpr == above / n, (target, above, k)
        if cal.threshold == -math.inf:
            assert k >= n
        else:
            lower = distinct[distinct < cal.threshold]
            nxt = lower[-1] if lower.size else -math.inf               # theta lowered to the next smaller distinct clean score
            assert int(np.count_nonzero(clean > nxt)) > k, (target, nxt)
    assert D.calibrate_threshold([0.3, 0.1, 0.2], 0.4).threshold == 0.2


# ------------------------------------------------------------------------------------------------------------ the hand-built example
CLEAN6, MARKED6 = [0.1, 0.3, 0.6], [0.4, 0.7, 0.9]
# thresholds  inf  .9  .7  .6  .4  .3  .1
# fp            0   0   0   1   1   2   3
# tp            0   1   2   2   3   3   3


def test_the_six_score_example():
    from awm_amd import detection as D
    curve = D.roc_curve(CLEAN6, MARKED6)
    assert list(curve.thresholds) == [math.inf, 0.9, 0.7, 0.6, 0.4, 0.3, 0.1]
    assert list(curve.fp) == [0, 0, 0, 1, 1, 2, 3] and list(curve.tp) == [0, 1, 2, 2, 3, 3, 3]
    assert D.auc_counts(curve) == (16, 18) and D.auc(curve) == 8 / 9   # 0.4 beats two clean scores, 0.7 and 0.9 all three
    assert D.eer(curve) == 1 / 3                                       # at threshold 0.6: FPR = 1/3 = FNR, a curve point
    assert D.tpr_at_fpr(curve, 0.0) == (2 / 3, 0.7)
    assert D.tpr_at_fpr(curve, 0.34) == (1.0, 0.4)
    assert D.tpr_at_fpr(curve, 0.3) == (2 / 3, 0.7)                    # 1/3 > 0.3: one false alarm is already too many
    assert D.tpr_at_fpr(curve, 1.0) == (1.0, 0.1)
    op = D.operating_point(CLEAN6, MARKED6, 0.5)
    assert (op["tp"], op["fp"], op["fn"], op["tn"]) == (2, 1, 1, 2)
    assert op["precision"] == 2 / 3 and op["recall"] == 2 / 3 and op["f1"] == 4 / 6 and op["accuracy"] == 4 / 6
    assert D.operating_point(CLEAN6, MARKED6, 0.6)["fp"] == 0, "the rule is score > threshold"
    # between curve points: clean .1 .5, marked .3 .5 .7 .9 -- FPR 0 0 0 .5 .5 1, FNR 1 .75 .5 .25 0 0; the segment from (0, .5) to
    # (.5, .25) crosses FPR = FNR at 1/3
    assert abs(D.eer(D.roc_curve([0.1, 0.5], [0.3, 0.5, 0.7, 0.9])) - 1 / 3) <= 1e-15
    assert D.eer(D.roc_curve([0.2], [0.1])) == 1.0


# ------------------------------------------------------------------------------------------------------------ the report
def test_detection_report_on_fabricated_pools():
    from awm_amd import detection as D
    clean = np.array([0.05, 0.10, 0.20, 0.30], np.float32)
    marked = np.array([0.25, 0.60, 0.70, 0.90], np.float32)
    biterr = np.array([0, 3, 0, 1])
    row = D.detection_report(marked, clean, biterr, 16, fpr_targets=(0.25, 0.5), threshold=0.5)
    assert list(row) == ["auc", "eer", "tpr_at_fpr", "deployed", "operating_point", "ber", "message_accuracy", "clips", "scores", "curve"]
    assert row["clips"] == 4 and row["ber"] == 4 / 64 and row["message_accuracy"] == 0.5
    assert row["auc"] == 15 / 16
    # one false alarm allowed of four: the lowest threshold with fp <= 1 is the marked score 0.25 (fp = 1: the clean 0.30), tp = 4
    assert row["tpr_at_fpr"][0.25] == (1.0, 0.25) and list(row["tpr_at_fpr"]) == [0.25, 0.5]
    assert row["tpr_at_fpr"][0.5] == (1.0, float(np.float32(0.2)))
    # its own calibration: k = 1 -> theta = the second largest clean score 0.2 -> marked above it: 4, clean above it: 1
    assert row["deployed"] == {0.25: (1.0, 0.25), 0.5: (1.0, 0.5)}
    assert row["operating_point"]["tp"] == 3 and row["operating_point"]["fp"] == 0
    assert row["scores"]["marked"] is not None and np.array_equal(row["scores"]["clean"], clean)
    # under an "attack" the clean scores rise; the deployed thresholds are the ones handed in, not this row's own
    none_thr = {0.25: D.calibrate_threshold(clean, 0.25).threshold, 0.5: D.calibrate_threshold(clean, 0.5).threshold}
    attacked = D.detection_report(marked - 0.1, clean + 0.2, biterr, 16, (0.25, 0.5), 0.5, deployed=none_thr)
    assert none_thr[0.25] == float(np.float32(0.2))
    assert attacked["deployed"][0.25] == (0.75, 1.0)                   # every attacked clean score is above 0.2
    assert attacked["tpr_at_fpr"][0.25][1] != none_thr[0.25]
    empty = D.detection_report(marked, clean, None, 0)
    assert math.isnan(empty["ber"]) and math.isnan(empty["message_accuracy"])
    with pytest.raises(ValueError):
        D.detection_report(marked, clean, biterr[:3], 16)


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_the_host_functions_check_their_arguments():
    from awm_amd import detection as D
    with pytest.raises(ValueError, match="2 of 3"):
        D.roc_curve([0.1, math.nan, math.inf], [0.5])
    with pytest.raises(ValueError, match="1 of 1"):
        D.roc_curve([0.1], [math.nan])
    with pytest.raises(ValueError):
        D.calibrate_threshold([0.1, math.inf], 0.1)
    with pytest.raises(ValueError):
        D.calibrate_threshold([], 0.1)
    with pytest.raises(ValueError):
        D.operating_point([0.1], [math.nan], 0.5)
    curve = D.roc_curve([0.1], [0.5])
    for bad in (-0.01, 1.01, math.nan, "0.1", True):
        with pytest.raises(ValueError):
            D.calibrate_threshold([0.1, 0.2], bad)
        with pytest.raises(ValueError):
            D.tpr_at_fpr(curve, bad)
        with pytest.raises(ValueError):
            D.evaluate_detection(None, None, [], fpr_targets=(bad,))
    with pytest.raises(ValueError, match="score"):
        D.evaluate_detection(None, None, [], score="logit")
    with pytest.raises(ValueError, match="decode"):
        D.evaluate_detection(None, None, [], decode="soft")
    with pytest.raises(ValueError, match="none"):
        D.evaluate_detection(None, None, [], attacks={"none": None})
    with pytest.raises(ValueError):
        D.evaluate_detection(None, None, [], threshold=1.5)
