"""wm_clip_scores on the GPU against the float64 yardstick (tests/detection_yardstick.py has the case table, the input builder and the
derivation of the floors), its special values, row independence and repeatability as bit patterns, every refusal through the raw C
ABI, and awm_amd.evaluate_detection end to end on the shipped Detector weights."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import detection_yardstick as DY
import loss_yardstick as LY
from gpu_support import awm, bits, dev, p, st  # noqa: F401
from oracle import wm_oracle as O

pytestmark = pytest.mark.gpu

INVALID = 1                                     # hipErrorInvalidValue


def _offset_by_one_float(x, dev):
    """x on the device at an address that is 4 (mod 16): a contiguous view one float into a fresh buffer"""
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(x.shape)
    view.copy_(x)
    return view


def _equal_ints(got, ref, B, what):
    assert np.array_equal(got.votes.cpu().numpy(), ref["votes"]), f"{what}: votes"
    assert np.array_equal(got.words.cpu().numpy(), ref["words"]), f"{what}: words"
    assert tuple(got.biterr.shape) == (B, 2) and np.array_equal(got.biterr.cpu().numpy(), ref["biterr"]), f"{what}: biterr"


# ------------------------------------------------------------------------------------------------------------ against the yardstick
@pytest.mark.parametrize("R,T,NO", DY.CASES)
def test_kernel_against_the_yardstick(awm, dev, R, T, NO):
    x, ref0, (p32, l32), bars = DY.case(R, T, NO)
    assert DY.soft_margin_ok(R, T, NO)                                 # so words[:, 1] may be compared as integers
    prob64, llr64 = torch.from_numpy(ref0["prob"]), torch.from_numpy(ref0["llr"])
    floors = {"prob": DY.PROB_FLOOR, "llr": DY.llr_floor(x.numpy())}
    first = None
    for aligned in (True, False):
        xd = x.to(dev) if aligned else _offset_by_one_float(x, dev)
        assert xd.data_ptr() % 16 == (0 if aligned else 4)
        for B in sorted({0, R // 2, R}):
            msg = DY.case_message(R, NO, B)
            for thr in DY.THR_LOGITS:
                prob_thr = 0.5 if thr == 0.0 else (0.0 if thr == -np.inf else (1.0 if thr == np.inf else 1.0 / (1.0 + math.exp(-thr))))
                thr_used = awm.ops.loc_threshold_logit(prob_thr)
                assert np.float32(thr_used) == np.float32(thr), "the probability stands for exactly this logit once it is a float32"
                ref = DY.clip_scores_ref(x.numpy(), msg.numpy(), thr_used) if (B or thr != 0.0) else ref0
                got = awm.ops.clip_scores(xd, msg.to(dev) if B else None, prob_thr)
                what = f"({R}, {T}, {NO}) aligned={aligned} B={B} thr={thr}"
                _equal_ints(got, ref, B, what)
                if first is None:
                    first = got
                    LY.held(got.prob.cpu(), prob64, p32, floors["prob"], what + " prob")
                    LY.held(got.llr.cpu(), llr64, l32, floors["llr"], what + " llr")
                else:                                                  # neither the alignment nor B nor the threshold moves a float bit
                    assert torch.equal(bits(got.prob), bits(first.prob)) and torch.equal(bits(got.llr), bits(first.llr)), what


# ------------------------------------------------------------------------------------------------------------ special values
def test_signed_zeros_cast_no_vote(awm, dev):
    x = torch.zeros(2, 100, 3)
    x[1] = -0.0
    got = awm.ops.clip_scores(x.to(dev), torch.tensor([3, 3]).to(dev))
    assert int(got.votes.abs().sum()) == 0 and int(got.words.abs().sum()) == 0
    assert got.biterr.cpu().tolist() == [[2, 2], [2, 2]]
    assert torch.equal(got.prob.cpu(), torch.full((2,), 0.5)) and torch.equal(got.llr.cpu(), torch.zeros(2, 3))


def test_infinities(awm, dev):
    x = DY.case_logits(3, 300, 5).clone()
    x[0, 7, 0] = math.inf
    x[1, 8, 0] = -math.inf
    x[2, 9, 2] = math.inf
    x[2, 10, 3] = -math.inf
    x[1, 11, 4] = math.inf
    x[1, 12, 4] = -math.inf                                            # both signs: the channel's llr is NaN, its soft bit 0
    ref = DY.clip_scores_ref(x.numpy(), None, 0.0)
    got = awm.ops.clip_scores(x.to(dev))
    _equal_ints(got, ref, 0, "infinities")
    prob, llr = got.prob.cpu().numpy(), got.llr.cpu().numpy()
    assert np.all(np.isfinite(prob)) and np.abs(prob - ref["prob"]).max() <= DY.PROB_FLOOR
    assert llr[0, 0] == math.inf and llr[1, 0] == -math.inf and llr[2, 2] == math.inf and llr[2, 3] == -math.inf and math.isnan(llr[1, 4])
    assert np.array_equal(np.isfinite(llr), np.isfinite(ref["llr"]))
    assert (int(got.words[2, 1]) >> 1) & 1 == 1 and (int(got.words[2, 1]) >> 2) & 1 == 0 and (int(got.words[1, 1]) >> 3) & 1 == 0
    for thr in (1.0, 0.0):                                             # thr_logit +inf: nothing votes; -inf: everything but -inf (not > -inf)
        v = awm.ops.clip_scores(x.to(dev), None, thr).votes[:, 0].cpu().tolist()
        assert v == ([0, 0, 0] if thr == 1.0 else [300, 299, 300]), (thr, v)


@pytest.mark.parametrize("channel", [0, 2])
def test_one_nan_stays_in_its_row_and_channel(awm, dev, channel):
    x = DY.case_logits(5, 4099, 17).clone()                           # 9 chunks a row; the NaN sits in the fourth
    msg = DY.case_message(5, 17, 5).to(dev)
    clean = awm.ops.clip_scores(x.to(dev), msg)
    t = 1700
    above = bool(x[3, t, channel] > 0)
    x[3, t, channel] = math.nan
    got = awm.ops.clip_scores(x.to(dev), msg)
    keep = [0, 1, 2, 4]
    for k in ("prob", "llr"):
        assert torch.equal(bits(getattr(got, k)[keep]), bits(getattr(clean, k)[keep])), k
    for k in ("votes", "words", "biterr"):
        assert torch.equal(getattr(got, k)[keep], getattr(clean, k)[keep]), k
    assert math.isnan(float(got.llr[3, channel])) and math.isnan(float(got.prob[3])) == (channel == 0)
    others = [o for o in range(17) if o != channel]
    assert torch.equal(bits(got.llr[3, others]), bits(clean.llr[3, others]))
    if channel != 0:
        assert torch.equal(bits(got.prob[3:4]), bits(clean.prob[3:4]))
    assert torch.equal(got.votes[3, others], clean.votes[3, others])
    assert int(got.votes[3, channel]) == int(clean.votes[3, channel]) - int(above), "the NaN casts no vote"
    ref = DY.clip_scores_ref(x.numpy(), msg.cpu().numpy(), 0.0)
    assert np.array_equal(got.votes.cpu().numpy(), ref["votes"]) and np.array_equal(got.words.cpu().numpy(), ref["words"])


# ------------------------------------------------------------------------------------------------------------ independence, repeatability
@pytest.mark.parametrize("R,T,NO", [(5, 4099, 17), (2, 4097, 64), (7, 1000, 1)])
def test_rows_are_independent_and_launches_repeat(awm, dev, R, T, NO):
    x = DY.case_logits(R, T, NO).to(dev)
    msg = DY.case_message(R, NO, R).to(dev)
    whole, again = awm.ops.clip_scores(x, msg, 0.7), awm.ops.clip_scores(x, msg, 0.7)
    for k in ("prob", "llr"):
        assert torch.equal(bits(getattr(whole, k)), bits(getattr(again, k))), k
    for k in ("votes", "words", "biterr"):
        assert torch.equal(getattr(whole, k), getattr(again, k)), k
    for r in range(R):                                                 # (rows of an odd length start at every alignment)
        one = awm.ops.clip_scores(x[r:r + 1], msg[r:r + 1], 0.7)
        for k in ("prob", "llr"):
            assert torch.equal(bits(getattr(one, k)), bits(getattr(whole, k)[r:r + 1])), (k, r)
        for k in ("votes", "words", "biterr"):
            assert torch.equal(getattr(one, k), getattr(whole, k)[r:r + 1]), (k, r)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_through_the_c_abi(awm, dev):
    dll = awm.lib.load()
    R, T, NO, B = 4, 100, 5, 2
    x = torch.zeros(R, T, NO, device=dev)
    msg = torch.zeros(B, dtype=torch.int64, device=dev)
    prob, llr = torch.empty(R, device=dev), torch.empty(R, NO, device=dev)
    votes = torch.empty(R, NO, dtype=torch.int32, device=dev)
    words = torch.empty(R, 2, dtype=torch.int64, device=dev)
    biterr = torch.empty(B, 2, dtype=torch.int32, device=dev)
    need = ctypes.c_longlong(0)
    assert dll.wm_clip_scores_plan(R, T, NO, ctypes.addressof(need), None) == 0 and need.value == R * 1 * (2 * NO + 1) * 4
    assert awm.ops.clip_scores_plan(3, 16000, 17) == 3 * 34 * 35 * 4
    scratch = torch.empty(need.value // 4, dtype=torch.int32, device=dev)
    good = dict(logits=p(x), message=p(msg), thr_logit=0.0, prob=p(prob), llr=p(llr), votes=p(votes), words=p(words), biterr=p(biterr),
                scratch=p(scratch), B=B, R=R, T=T, NO=NO)

    def call(**kw):
        a = dict(good, **kw)
        return dll.wm_clip_scores(a["logits"], a["message"], a["thr_logit"], a["prob"], a["llr"], a["votes"], a["words"], a["biterr"],
                                  a["scratch"], a["B"], a["R"], a["T"], a["NO"], st())
    assert call() == 0
    assert call(prob=None, llr=None, words=None, biterr=None, message=None, B=0) == 0, "every output but votes is optional"
    bad = {
        "R < 1": dict(R=0, B=0), "T < 1": dict(T=0), "NO < 1": dict(NO=0), "NO > 64": dict(NO=65), "B < 0": dict(B=-1), "B > R": dict(B=R + 1),
        "R T NO > 2^46": dict(R=2 ** 40, T=2 ** 6 + 1, NO=1), "T > 2^24": dict(T=2 ** 24 + 1, R=1, B=0, NO=1), "NaN threshold": dict(thr_logit=math.nan),
        "null logits": dict(logits=None), "null votes": dict(votes=None), "null scratch": dict(scratch=None),
        "misaligned logits": dict(logits=p(x) + 2), "misaligned prob": dict(prob=p(prob) + 2), "misaligned words": dict(words=p(words) + 4),
        "misaligned message": dict(message=p(msg) + 4, B=1), "misaligned scratch": dict(scratch=p(scratch) + 1),
        "votes on the input": dict(votes=p(x)), "prob inside the input": dict(prob=p(x) + 16), "scratch on the input": dict(scratch=p(x)),
        "biterr on the message": dict(biterr=p(msg)), "llr on votes": dict(llr=p(votes)), "prob on words": dict(prob=p(words)),
        "scratch on llr": dict(scratch=p(llr)),
    }
    for what, kw in bad.items():
        assert call(**kw) == INVALID, what
    for what, a in {"R < 1": (0, T, NO), "T < 1": (R, 0, NO), "NO > 64": (R, T, 65), "T > 2^24": (1, 2 ** 24 + 1, 1),
                    "R T NO > 2^46": (2 ** 40, 2 ** 6 + 1, 1)}.items():
        assert dll.wm_clip_scores_plan(*a, ctypes.addressof(need), None) == INVALID, what
    assert dll.wm_clip_scores_plan(R, T, NO, None, None) == INVALID
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ evaluate_detection
def _models(awm, dev):
    ck = np.load(os.path.join(os.path.dirname(__file__), "golden", "detector_best_unprefixed.npz"))
    D = awm.Detector(16)
    D.load_state_dict({k: torch.from_numpy(ck[k]) for k in ck.files})
    torch.manual_seed(17)
    G = awm.Generator(16)
    return G.to(dev).eval(), D.to(dev).eval()


def test_evaluate_detection_end_to_end(awm, dev):
    from awm_amd import detection as Dt
    G, D = _models(awm, dev)
    batches = [O.synthetic_clips(2, seed=51, T=2048), O.synthetic_clips(2, seed=52, T=2048)]
    messages = [torch.tensor([3, 60001]), torch.tensor([77, 12345])]

    def noise():
        return {"noise": awm.Distortion(gain_db=0, snr_db=10)}
    atk = noise()
    res = awm.evaluate_detection(G, D, batches, atk, device=dev, messages=messages, fpr_targets=(0.01, 0.5))
    print({k: {kk: vv for kk, vv in v.items() if kk not in ("scores", "curve")} for k, v in res.items()})
    assert list(res) == ["none", "noise"]
    assert atk["noise"].draw == 2, "one call per batch, on the concatenation of s + delta and s"
    # the same Detector outputs, scored directly
    direct = {"none": ([], [], []), "noise": ([], [], [])}
    fresh, prob_bar = noise(), 0.0
    with torch.no_grad():
        for s, m in zip(batches, messages):
            s, m = s.to(dev), m.to(dev)
            both = torch.cat([s + awm.postprocess(G(s, m)), s], dim=0)
            for name, x in (("none", both), ("noise", fresh["noise"](both))):
                lg = D(x)
                cs = awm.ops.clip_scores(lg, m, 0.5)
                ref64 = DY.clip_scores_ref(lg.cpu().numpy())["prob"]
                prob_bar = max(prob_bar, 8 * DY.rel_err(DY.torch32(lg.cpu())[0].numpy(), ref64), DY.PROB_FLOOR)
                LY.held(cs.prob.cpu(), torch.from_numpy(ref64), DY.torch32(lg.cpu())[0], DY.PROB_FLOOR, f"{name} prob on the Detector's logits")
                direct[name][0].append(cs.prob[:2]); direct[name][1].append(cs.prob[2:]); direct[name][2].append(cs.biterr[:, 0])
    none_clean = torch.cat(direct["none"][1]).cpu().numpy()
    for name, row in res.items():
        marked, clean, be = (torch.cat(v).cpu().numpy() for v in direct[name])
        assert row["clips"] == 4
        assert row["scores"]["marked"].dtype == np.float32
        assert np.array_equal(row["scores"]["marked"].view(np.int32), marked.view(np.int32)), name
        assert np.array_equal(row["scores"]["clean"].view(np.int32), clean.view(np.int32)), name
        curve = Dt.roc_curve(clean, marked)
        assert all(np.array_equal(a, b) for a, b in zip(row["curve"][:3], curve[:3])) and row["curve"][3:] == curve[3:]
        assert row["auc"] == Dt.auc(curve) and row["eer"] == Dt.eer(curve)
        assert dict(row["tpr_at_fpr"]) == {t: Dt.tpr_at_fpr(curve, t) for t in (0.01, 0.5)}
        theta = {t: Dt.calibrate_threshold(none_clean, t).threshold for t in (0.01, 0.5)}
        assert dict(row["deployed"]) == {t: (float(np.mean(marked > theta[t])), float(np.mean(clean > theta[t]))) for t in (0.01, 0.5)}
        assert row["ber"] == be.sum() / 64 and row["message_accuracy"] == float(np.mean(be == 0))
        assert dict(row["operating_point"]) == dict(Dt.operating_point(clean, marked, 0.5))
        flat = [row["auc"], row["eer"], row["ber"], row["message_accuracy"], row["operating_point"]["accuracy"], row["operating_point"]["recall"]]
        flat += [v for t in row["tpr_at_fpr"].values() for v in t[:1]] + [v for t in row["deployed"].values() for v in t]
        assert all(math.isfinite(v) for v in flat), (name, flat)
    # against the mean probabilities of evaluate_robustness on fresh attack objects: the same clips, torch's reductions
    rob = awm.evaluate_robustness(G, D, batches, noise(), device=dev, messages=messages)
    for name, row in res.items():
        for key, half in (("watermarked_prob", "marked"), ("clean_prob", "clean")):
            mean = float(row["scores"][half].astype(np.float64).mean())
            # prob_bar: the rule's bar on these very logits (relative to the largest clip score, at most 1)
            print(f"{name} {key}: {mean!r} against {rob[name][key]!r}, bar {prob_bar:.3e}")
            assert abs(mean - rob[name][key]) <= prob_bar * float(row["scores"][half].max()), (name, key, mean, rob[name][key])
    # the other score and the other decoder: the call runs, and only the documented entries move
    alt = awm.evaluate_detection(G, D, batches, noise(), device=dev, messages=messages, fpr_targets=(0.01, 0.5), score="vote", decode="llr")
    assert list(alt) == ["none", "noise"]
    for name in alt:
        assert alt[name]["clips"] == 4 and alt[name]["scores"]["marked"].dtype == np.float64
        assert np.all((alt[name]["scores"]["marked"] * 2048) % 1 == 0), "a vote score is a count over T"
    only_decode = awm.evaluate_detection(G, D, batches, noise(), device=dev, messages=messages, fpr_targets=(0.01, 0.5), decode="llr")
    for name, row in res.items():
        for k in row:
            if k in ("ber", "message_accuracy"):
                continue
            a, b = row[k], only_decode[name][k]
            if k == "scores":
                assert all(np.array_equal(a[h], b[h]) for h in a)
            elif k == "curve":
                assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3])) and a[3:] == b[3:]
            else:
                assert a == b, (name, k)


def test_evaluate_detection_without_a_message(awm, dev):
    torch.manual_seed(3)
    G, D = awm.Generator(0).to(dev).eval(), awm.Detector(0).to(dev).eval()
    res = awm.evaluate_detection(G, D, [O.synthetic_clips(2, seed=5, T=2048)], device=dev, message_bits=0)
    assert list(res) == ["none"] and res["none"]["clips"] == 2
    assert math.isnan(res["none"]["ber"]) and math.isnan(res["none"]["message_accuracy"]) and math.isfinite(res["none"]["auc"])
