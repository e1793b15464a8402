"""wm_stoi / ops.stoi / awm_amd.stoi and the quality columns of the evaluation entry points on the GPU against the float64 yardstick of
tests/stoi_yardstick.py (numpy from the definition in include/wm_hip.h; nothing from the package).  Three rows a launch, x and y one
float into their buffers.

Bars (none tuned to the kernel):
  kept       exact.  Precondition, asserted on the yardstick: no frame of a row lies within 0.01 dB of the silence threshold (the recipe's
             smallest margin is 0.47 dB; a float32 frame energy is good to about 1e-5 dB), so no case is excused for a mask flip.
  sentinel   rows with fewer than 30 spectral frames: exactly 1e-5 (as float32).
  floats     |d - d64| <= 8 x max over this file's rows of |d_twin - d64|  +  16 x 2^-24.  The twin is the yardstick's float32 restatement:
             what float32 costs in some order; the factor 8 covers a summation and transform order different from the twin's, the floor is
             the float32 rounding of a final tree mean of at most 2^11 terms of magnitude <= 1, rounded up.
  bits       rows alone / in another place of another batch / in a second launch, the 16 kHz path against resample_rows + the 10 kHz
             path, and the plumbing against direct ops.stoi calls: identical bits.
Every reference is computed once (lru_cache in the yardstick) and never written to.

Measured on an MI355X (largest err / bound per case, printed by every case): see DESIGN.md section 4j."""
import numpy as np
import pytest
import torch

from oracle import wm_oracle as O

import stoi_yardstick as Y
from gpu_support import awm, dev  # noqa: F401
from gpu_support import bits, reference_models

pytestmark = pytest.mark.gpu

SENTINEL32 = float(np.float32(Y.SENTINEL))


def off_by_one_float(a, dev):
    """the same values in a buffer that starts 4 bytes earlier: the returned tensor's pointer is 4 (mod 8)"""
    a = np.array(a, dtype=np.float32, order="C")                  # a copy: the yardstick's cases are read-only
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
    buf[1:] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[1:].view(a.shape)


def launch(dev, x, y):
    from awm_amd import ops
    xd, yd = off_by_one_float(x, dev), off_by_one_float(y, dev)
    assert xd.data_ptr() % 8 == 4 and yd.data_ptr() % 8 == 4
    d, kept = ops.stoi(xd, yd, 10000)
    assert d.dtype == torch.float32 and kept.dtype == torch.int32 and tuple(d.shape) == (len(x),) == tuple(kept.shape)
    return d.cpu().numpy(), kept.cpu().numpy()


def twin_error():
    """max |d_twin - d64| over the float cases of this file"""
    worst = 0.0
    for n, kind in Y.FLOAT_CASES:
        r64, r32 = Y.case_ref(n, kind)
        worst = max(worst, max(abs(a.d - b.d) for a, b in zip(r64, r32)))
    return worst


def bar():
    return 8.0 * twin_error() + 16.0 * 2.0 ** -24


# ------------------------------------------------------------------------------------------ 1. accuracy at 10 kHz
@pytest.mark.parametrize("n,kind", Y.SENTINEL_CASES)
def test_short_rows_give_the_sentinel_exactly(awm, dev, n, kind):
    x, y = Y.case(n, kind)
    ref = [Y.stoi(a, b) for a, b in zip(x, y)]
    assert all(s.d == Y.SENTINEL and s.margin_db > 0.01 for s in ref)
    d, kept = launch(dev, x, y)
    print(f"n {n} {kind}: kept {kept.tolist()}, wanted {[s.K for s in ref]}")
    assert kept.tolist() == [s.K for s in ref]
    assert d.tolist() == [SENTINEL32] * 3


@pytest.mark.parametrize("n,kind", Y.FLOAT_CASES)
def test_scores_against_float64(awm, dev, n, kind):
    x, y = Y.case(n, kind)
    r64, _ = Y.case_ref(n, kind)
    assert all(s.margin_db > 0.01 for s in r64), "precondition: no frame within 0.01 dB of the silence threshold"
    assert all(s.K > 30 for s in r64), "every row has a segment"
    if n == 4097:
        assert all(s.K == 31 for s in r64), "exactly one segment"
    d, kept = launch(dev, x, y)
    err = np.abs(d.astype(np.float64) - np.array([s.d for s in r64]))
    print(f"n {n} {kind}: d {d.tolist()}, kept {kept.tolist()}, worst err {err.max():.3e}, bar {bar():.3e}, err / bound {err.max() / bar():.4f}")
    assert kept.tolist() == [s.K for s in r64], "the kept-frame count is exact"
    assert (err <= bar()).all()


# ------------------------------------------------------------------------------------------ 2. exact cases
def test_all_zero_rows_score_exactly_zero(awm, dev):
    x, y = Y.case(6250, "speech")
    z = np.zeros_like(x[0])
    d, kept = launch(dev, np.stack([z, x[1], z]), np.stack([y[0], z, z]))
    assert d.tolist() == [0.0, 0.0, 0.0] and np.isfinite(d).all()
    assert kept.tolist() == [Y.frame_count(6250), Y.stoi(x[1], z).K, Y.frame_count(6250)]


@pytest.mark.parametrize("where", ["x", "y"])
def test_a_nan_sample_spoils_its_row_alone(awm, dev, where):
    x, y = Y.case(6250, "speech")
    d0, k0 = launch(dev, x, y)
    for pos in (0, 3000, 6249):                          # the first sample, one in the middle, one behind the last frame
        bad = np.array(y if where == "y" else x)
        bad[1, pos] = np.nan
        d, kept = launch(dev, bad if where == "x" else x, bad if where == "y" else y)
        assert np.isnan(d[1]) and kept[1] == 0, f"{where}[{pos}]"
        assert d[0].tobytes() == d0[0].tobytes() and d[2].tobytes() == d0[2].tobytes() and kept[0] == k0[0] and kept[2] == k0[2]


# ------------------------------------------------------------------------------------------ 3. independence
@pytest.mark.parametrize("n", [4097, 20000])
def test_rows_are_independent_and_launches_reproducible(awm, dev, n):
    from awm_amd import ops
    kind = "noise" if n == 4097 else "speech"
    x, y = Y.case(n, kind)
    xd, yd = off_by_one_float(x, dev), off_by_one_float(y, dev)
    d, kept = ops.stoi(xd, yd, 10000)
    d2, kept2 = ops.stoi(xd, yd, 10000)
    assert torch.equal(bits(d), bits(d2)) and torch.equal(kept, kept2), "two launches give identical bits"
    alone = ops.stoi(xd[1:2].clone(), yd[1:2].clone(), 10000)
    first = ops.stoi(xd[[1, 0, 2]], yd[[1, 0, 2]], 10000)
    other = Y.case(n, "noise" if kind == "speech" else "speech")
    x5 = torch.cat([off_by_one_float(other[0], dev), xd[2:3], xd[1:2]])
    y5 = torch.cat([off_by_one_float(other[1], dev), yd[2:3], yd[1:2]])
    last = ops.stoi(x5, y5, 10000)
    for got, r in ((alone, 0), (first, 0), (last, 4)):
        assert torch.equal(bits(got[0][r]), bits(d[1])) and int(got[1][r]) == int(kept[1]), "a row's bits know nothing of the batch"


# ------------------------------------------------------------------------------------------ 4. rates
def test_16k_is_one_resampling_launch_then_the_10k_path(awm, dev):
    from awm_amd import ops
    rng = np.random.default_rng(21)
    x16 = np.stack([Y.speech_like(16000, 40 + i) for i in range(3)])
    y16 = x16 + (0.02 * rng.standard_normal(x16.shape)).astype(np.float32)
    xd, yd = off_by_one_float(x16, dev), off_by_one_float(y16, dev)
    got = ops.stoi(xd, yd, 16000)
    x10, y10 = ops.resample_rows(xd, 16000, 10000), ops.resample_rows(yd, 16000, 10000)
    assert x10.shape[1] == 10000
    want = ops.stoi(x10, y10, 10000)
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1])
    assert torch.equal(bits(ops.stoi(xd, yd)[0]), bits(got[0])), "16 kHz is the default"
    ref = [Y.stoi(a, b) for a, b in zip(x10.cpu().numpy(), y10.cpu().numpy())]
    assert all(s.margin_db > 0.01 for s in ref)
    err = np.abs(got[0].cpu().numpy().astype(np.float64) - np.array([s.d for s in ref]))
    print(f"16 kHz rows: d {got[0].tolist()}, err / bound {err.max() / bar():.4f}")
    assert got[1].tolist() == [s.K for s in ref] and (err <= bar()).all() and all(s.K > 30 for s in ref)


# ------------------------------------------------------------------------------------------ 5. plumbing
def test_public_stoi_keeps_the_leading_shape(awm, dev):
    from awm_amd import ops
    x, y = Y.case(6250, "speech")
    xd, yd = off_by_one_float(x, dev), off_by_one_float(y, dev)
    want = ops.stoi(xd, yd, 10000)[0]
    for a, b, shape in ((xd[:, None], yd[:, None], (3,)), (xd, yd, (3,)), (xd[2], yd[2], ())):
        got = awm.stoi(a, b, 10000)
        assert tuple(got.shape) == shape and got.is_cuda and got.dtype == torch.float32
        assert torch.equal(bits(got.reshape(-1)), bits(want if shape else want[2:3]))
    cpu = awm.stoi(xd.cpu(), yd.cpu(), 10000)
    assert not cpu.is_cuda and float((cpu - want.cpu()).abs().max()) <= bar(), "the host path is the float64 restatement"


def test_evaluate_robustness_quality_columns(awm, dev):
    from awm_amd import ops
    G, D = reference_models(awm, dev)
    B, T = 4, 16000
    batches = [O.synthetic_clips(B, seed=71, T=T)]
    messages = [torch.tensor([3, 60001, 77, 12345])]

    def attacks():
        return {"noise": awm.Distortion(gain_db=0, snr_db=10)}
    old = awm.evaluate_robustness(G, D, batches, attacks(), device=dev, messages=messages)
    res = awm.evaluate_robustness(G, D, batches, attacks(), device=dev, messages=messages, quality=("stoi",))
    print(res)
    four = ["bit_accuracy", "clean_prob", "delta_rms", "watermarked_prob"]
    assert list(res) == list(old) == ["none", "noise"]
    for name in res:
        assert sorted(old[name]) == four and sorted(res[name]) == sorted(four + ["stoi", "stoi_attack_only", "stoi_rows"])
        for k in four:
            assert res[name][k] == old[name][k], "the old columns are the old numbers"
    # the same tensors, by hand
    s = batches[0].to(dev)
    G.eval()
    with torch.no_grad():
        delta = awm.postprocess(G(s, messages[0].to(dev)))
    both = torch.cat([s + delta, s], dim=0)
    ref2 = torch.cat([s, s], dim=0)
    for name, attacked in (("none", both), ("noise", attacks()["noise"](both))):
        d, kept = ops.stoi(ref2, attacked)
        scored = kept[:B] > 30
        assert int(scored.sum()) == res[name]["stoi_rows"] > 0
        assert res[name]["stoi"] == float(d[:B][scored].double().mean()), "bit for bit a direct ops.stoi on the same tensors"
        assert res[name]["stoi_attack_only"] == float(d[B:][scored].double().mean())
    assert abs(res["none"]["stoi_attack_only"] - 1.0) <= bar(), "the clean half of the undistorted row is s against s"
    assert res["noise"]["stoi_attack_only"] < res["none"]["stoi_attack_only"]
    with pytest.raises(ValueError, match="unknown metric"):
        awm.evaluate_robustness(G, D, batches, attacks(), device=dev, messages=messages, quality=("pesq",))


def test_file_level_stoi(awm, dev):
    from awm_amd import ops
    G, D = reference_models(awm, dev)
    n = 51200                                            # 3.2 s at 16 kHz: three whole segments and a remainder
    wave = O.synthetic_clips(4, seed=81, T=16000).reshape(1, -1)[:, :n].contiguous()
    torch.manual_seed(5)
    res = awm.generate_watermarked_audio(wave, G, device=dev, stoi=True)
    torch.manual_seed(5)
    plain = awm.generate_watermarked_audio(wave, G, device=dev)
    assert "stoi" not in plain["metrics"] and sorted(plain["metrics"]) == ["power_ratio_db", "si_snr_db", "watermark_rms"]
    assert torch.equal(plain["watermarked_waveform"], res["watermarked_waveform"])
    for k in plain["metrics"]:
        assert plain["metrics"][k] == res["metrics"][k]
    d, kept = ops.stoi(res["original_waveform"].to(dev), res["watermarked_waveform"].to(dev), 16000)
    assert tuple(d.shape) == (1,) and int(kept[0]) > 30
    assert res["metrics"]["stoi"] == float(d[0]) and 0.0 < res["metrics"]["stoi"] <= 1.0 + bar()
    msgs = torch.tensor([1, 2, 3, 4])
    five = awm.evaluate_unseen_file(wave, G, D, device=dev, messages=msgs, stoi=True)
    four = awm.evaluate_unseen_file(wave, G, D, device=dev, messages=msgs)
    assert len(four) == 4 and len(five) == 5
    assert all(a == b or (a != a and b != b) for a, b in zip(four, five[:4]))
    with torch.no_grad():
        segs = torch.nn.functional.pad(wave, (0, 64000 - n)).reshape(4, 1, 16000).to(dev)
        G.eval()
        wm = (segs + G(segs, msgs.to(dev))).reshape(1, -1)[:, :n]
    want = ops.stoi(wave.to(dev), wm.contiguous(), 16000)[0]
    assert five[4] == float(want[0])


# ------------------------------------------------------------------------------------------ 6. refusals
def test_bad_arguments(awm, dev):
    from awm_amd import ops
    st = torch.cuda.current_stream().cuda_stream
    x, y = torch.zeros(3, 5000, device=dev), torch.zeros(3, 5000, device=dev)
    d, kept = torch.zeros(3, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)
    sc = torch.zeros(ops.stoi_plan(3, 5000) // 4, device=dev)
    px, py, pd, pk, ps = (t.data_ptr() for t in (x, y, d, kept, sc))
    for args in ((px, py, pd, pk, ps, 0, 5000, st), (px, py, pd, pk, ps, 3, 0, st), (px, py, pd, pk, ps, 3, 2 ** 34 + 1, st),
                 (None, py, pd, pk, ps, 3, 5000, st), (px, py, None, pk, ps, 3, 5000, st), (px, py, pd, pk, None, 3, 5000, st),
                 (px + 2, py, pd, pk, ps, 3, 5000, st), (px, py, pd, pk, ps + 1, 3, 5000, st),
                 (px, py, px, pk, ps, 3, 5000, st), (px, py, pd, pk, py, 3, 5000, st), (px, py, pd, pd, ps, 3, 5000, st)):
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm.lib.wm_stoi(*args)
    with pytest.raises(ValueError):
        ops.stoi(x, y[:, :-1], 10000)
    with pytest.raises(ValueError):
        ops.stoi(x, y.cpu(), 10000)
    with pytest.raises(ValueError):
        ops.stoi(x.double(), y.double(), 10000)
    torch.cuda.synchronize()
