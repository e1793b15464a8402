"""wm_masking_fwd / wm_masking_bwd, awm_amd.masking / MaskingLoss / nmr and their wiring on the GPU against the float64 yardstick of
tests/masking_yardstick.py (numpy from the definition in include/wm_hip.h; nothing from the package).  x and y one float into their
buffers.

Bars (none tuned to the kernel):
  counts     audible and cells exact.  Precondition, asserted on the float64 model: no cell of a row has |r - 1| < 1e-4 (about 100 x the
             float32 floor of r), so no case is excused for a cell on the hinge; the gradient comparison stands on the same precondition
             (the active set is the same).
  floats     8 x the error of the yardstick's own float32 mode against its float64 mode on the launch's own rows: absolute for nmr_db and
             over_db, relative L2 for a row's gradient.  The 8 covers a radix-2 butterfly and tree reductions that order sums differently
             from a matrix product, and the device's logf / expf.  Rows whose float64 gradient is zero must come back as exact zeros.
  bits       two launches, a row alone / first of three / last of five, autograd against the direct call, the plumbing against direct
             masking calls: identical bits.
Every reference is computed once (lru_cache in the yardstick) and never written to.

Measured on an MI355X (floors, errors and err / bar per case, printed by every case): see DESIGN.md section 4u."""
import copy
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import wm_oracle as O

import masking_yardstick as Y
from gpu_support import awm, dev  # noqa: F401
from gpu_support import bits, reference_models

pytestmark = pytest.mark.gpu


def M():
    return importlib.import_module("awm_amd.masking")


def off_by_one_float(a, dev):
    """the same values in a buffer that starts 4 bytes earlier: the returned tensor's pointer is 4 (mod 8)"""
    a = np.array(a, dtype=np.float32, order="C")                  # a copy: the yardstick's cases are read-only
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
    buf[1:] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[1:].view(a.shape)


def raw(awm, xd, yd, gout=None):
    """the two C calls on contiguous device rows: (nmr_db, over_db, counts (rows, 2), coef, gy); gout = 1 for every row by default"""
    rows, n = xd.shape
    frames, _, need = M().masking_plan(rows, n)
    dev = xd.device
    nmr, over = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    counts = torch.empty(rows, 2, dtype=torch.int32, device=dev)
    coef = torch.empty(rows, frames, 22, device=dev)
    scratch = torch.empty(need // 4, dtype=torch.int32, device=dev)
    tab = M().masking_tables()["packed"].to(dev)
    st = torch.cuda.current_stream().cuda_stream
    awm.lib.wm_masking_fwd(xd.data_ptr(), yd.data_ptr(), tab.data_ptr(), nmr.data_ptr(), over.data_ptr(), counts.data_ptr(), coef.data_ptr(),
                           scratch.data_ptr(), rows, n, st)
    gout = torch.ones(rows, device=dev) if gout is None else gout
    gy = torch.full_like(yd, 7.0).contiguous()                    # every sample must be written
    awm.lib.wm_masking_bwd(xd.data_ptr(), yd.data_ptr(), coef.data_ptr(), gout.data_ptr(), gy.data_ptr(), rows, n, st)
    return nmr, over, counts, coef, gy


def compare(label, got, refs, floors):
    """the launch's five results against the float64 Results, at 8 x the floors"""
    nmr, over, counts, _, gy = (t.cpu().numpy() for t in got)
    fn, fo, fg = floors
    worst = [0.0, 0.0, 0.0]
    for i, r in enumerate(refs):
        assert Y.hinge_distance(r) > Y.HINGE_MARGIN, "precondition: no cell within 1e-4 of the hinge"
        assert counts[i].tolist() == [r.audible, r.cells], (label, i, counts[i].tolist(), r.audible, r.cells)
        if math.isnan(r.nmr_db):
            assert math.isnan(nmr[i])
        elif math.isinf(r.nmr_db):
            assert nmr[i] == r.nmr_db
        else:
            worst[0] = max(worst[0], abs(float(nmr[i]) - r.nmr_db))
        worst[1] = max(worst[1], abs(float(over[i]) - r.over_db))
        if np.any(r.grad):
            worst[2] = max(worst[2], float(np.linalg.norm(gy[i].astype(np.float64) - r.grad) / np.linalg.norm(r.grad)))
        else:
            assert not gy[i].any(), "a zero gradient is exact zeros"
        tail = Y.HOP * (Y.frame_count(gy.shape[1]) + 1) if Y.frame_count(gy.shape[1]) else 0
        assert not gy[i, tail:].any(), "samples no frame covers get 0"
    print(f"{label}: floors nmr {fn:.2e} over {fo:.2e} grad {fg:.2e} | errors nmr {worst[0]:.2e} over {worst[1]:.2e} grad {worst[2]:.2e} | "
          f"err / bar {worst[0] / (8 * fn + 1e-300):.3f} {worst[1] / (8 * fo + 1e-300):.3f} {worst[2] / (8 * fg + 1e-300):.3f}")
    assert worst[0] <= 8 * fn and worst[1] <= 8 * fo and worst[2] <= 8 * fg


def size(awm, label):
    chunk = M().masking_plan(1, 16000)[1]
    return {"seam": 256 * (chunk - 1) + 512, "seam+hop": 256 * chunk + 512, "two chunks+1": 256 * (2 * chunk) + 512 + 1}.get(label, label)


# ------------------------------------------------------------------------------------------ 1. shapes and accuracy
@pytest.mark.parametrize("label", [511, 512, 767, 768, 1280, "seam", "seam+hop", "two chunks+1", 16000])
def test_three_rows_against_float64(awm, dev, label):
    n = size(awm, label)
    x, y = Y.case(n)
    r64, _ = Y.case_ref(n)
    xd, yd = off_by_one_float(x, dev), off_by_one_float(y, dev)
    assert xd.data_ptr() % 8 == 4 and yd.data_ptr() % 8 == 4
    got = raw(awm, xd, yd)
    if n == 511:
        assert M().masking_plan(3, n)[0] == 0 and all(r.cells == 0 for r in r64)
    compare(f"n {n}", got, r64, Y.floors(n))
    res = awm.masking(xd, yd)
    assert torch.equal(bits(res.nmr_db), bits(got[0])) and torch.equal(bits(res.over_db), bits(got[1]))
    assert torch.equal(res.audible, got[2][:, 0]) and torch.equal(res.cells, got[2][:, 1]) and res.cells.dtype == torch.int32


def test_one_long_row_from_offset_pointers(awm, dev):
    n = 16000 * 4 + 13
    x, y = Y.case(n)
    r64, _ = Y.case_ref(n)
    xd, yd = off_by_one_float(x[1:2], dev), off_by_one_float(y[1:2], dev)
    assert xd.data_ptr() % 8 == 4 and r64[1].cells == 22 * 249
    compare(f"n {n} one row", raw(awm, xd, yd), r64[1:2], Y.floors(n, rows=(1,)))


# ------------------------------------------------------------------------------------------ 2. edge rows
def test_edge_rows(awm, dev):
    n = 1280
    x, y = Y.case(n)
    # no difference: -inf, 0 and a zero gradient; a silent reference: the threshold in quiet only
    xs = np.stack([x[0], np.zeros(n, dtype=np.float32), x[2]])
    ys = np.stack([x[0], y[1] - x[1], y[2]])
    refs = [Y.model(a, b) for a, b in zip(xs, ys)]
    floors = Y.floors_of(refs, [Y.model(a, b, twin=True) for a, b in zip(xs, ys)])
    got = raw(awm, off_by_one_float(xs, dev), off_by_one_float(ys, dev))
    assert refs[0].nmr_db == -math.inf and refs[0].over_db == 0.0 and refs[1].audible > 0
    assert float(got[0][0]) == -math.inf and float(got[1][0]) == 0.0 and got[2][0].tolist() == [0, 88] and not got[4][0].any()
    compare("edge rows", got, refs, floors)
    # one NaN sample between two clean rows: that row is NaN / 0, its neighbours are the bits of a launch without it
    clean = raw(awm, off_by_one_float(x, dev), off_by_one_float(y, dev))
    for where, pos in (("x", 0), ("y", 700), ("y", n - 1), ("x", n - 1)):
        xb, yb = np.array(x), np.array(y)
        (xb if where == "x" else yb)[1, pos] = np.nan
        bad = raw(awm, off_by_one_float(xb, dev), off_by_one_float(yb, dev))
        assert math.isnan(float(bad[0][1])) and math.isnan(float(bad[1][1])) and bad[2][1].tolist() == [0, 0], (where, pos)
        for i in (0, 2):
            assert all(torch.equal(bits(a[i].float()), bits(b[i].float())) for a, b in zip(bad, clean)), (where, pos, i)


# ------------------------------------------------------------------------------------------ 3. determinism and independence
def test_rows_are_independent_and_launches_reproducible(awm, dev):
    n = size(awm, "two chunks+1")
    x, y = Y.case(n)
    xd, yd = off_by_one_float(x, dev), off_by_one_float(y, dev)
    g3 = torch.tensor([0.5, -2.0, 3.0], device=dev)
    one, two = raw(awm, xd, yd, g3), raw(awm, xd, yd, g3)
    assert all(torch.equal(bits(a.float()), bits(b.float())) for a, b in zip(one, two)), "two launches give identical bits"
    assert one[2][1, 0] > 0 and one[4][1].any()
    ox, oy = Y.case(size(awm, "seam"))
    pad = lambda a: np.pad(a[:2], ((0, 0), (0, n - a.shape[1])))                  # noqa: E731  two other rows, as long as these
    alone = raw(awm, xd[1:2].clone(), yd[1:2].clone(), g3[1:2].clone())
    first = raw(awm, xd[[1, 0, 2]], yd[[1, 0, 2]], g3[[1, 0, 2]])
    x5 = torch.cat([off_by_one_float(pad(ox), dev), xd[[2, 0, 1]]])
    y5 = torch.cat([off_by_one_float(pad(oy), dev), yd[[2, 0, 1]]])
    last = raw(awm, x5, y5, torch.tensor([1.0, 1.0, 3.0, 0.5, -2.0], device=dev))
    for got, r in ((alone, 0), (first, 0), (last, 4)):
        assert all(torch.equal(bits(a[r].float()), bits(b[1].float())) for a, b in zip(got, one)), "a row's bits know nothing of the batch"


# ------------------------------------------------------------------------------------------ 4. autograd
def test_loss_backward_is_the_direct_call(awm, dev):
    n = 767
    x, y = Y.case(1280)
    xd, yd = off_by_one_float(x[:, :n], dev), off_by_one_float(y[:, :n], dev)
    yl = yd[:, None].clone().requires_grad_(True)
    xl = xd[:, None].clone().requires_grad_(True)
    loss = awm.MaskingLoss()(xl, yl)
    loss.backward()
    nmr, over, counts, coef, gy = raw(awm, xd, yd, torch.ones(3, device=dev) / 3)
    assert torch.equal(bits(loss.detach().reshape(1)), bits(over.mean().reshape(1))) and xl.grad is None
    assert tuple(yl.grad.shape) == (3, 1, n) and torch.equal(bits(yl.grad[:, 0]), bits(gy)) and gy[2].any()
    assert not yl.grad[:, 0, 512:].any(), "exactly 0 on the unjudged tail"
    host = awm.MaskingLoss()(xd.cpu(), yd.cpu())
    assert abs(float(host) - float(loss.detach())) <= 1e-5, "the host path is the float64 restatement"


# ------------------------------------------------------------------------------------------ 5. plumbing
def test_public_entry_points_keep_the_leading_shape(awm, dev):
    x, y = Y.case(1280)
    xd, yd = off_by_one_float(x, dev), off_by_one_float(y, dev)
    want = awm.masking(xd, yd)
    for a, b, shape in ((xd[:, None], yd[:, None], (3,)), (xd, yd, (3,)), (xd[2], yd[2], ())):
        got = awm.nmr(a, b)
        assert tuple(got.shape) == shape and got.is_cuda and got.dtype == torch.float32
        assert torch.equal(bits(got.reshape(-1)), bits(want.nmr_db if shape else want.nmr_db[2:3]))
    at8 = awm.masking(xd[:, ::2].contiguous(), yd[:, ::2].contiguous(), 8000)      # another rate: one resampling launch, then the 16 kHz path
    from awm_amd import ops
    up = ops.resample_rows(torch.cat([xd[:, ::2], yd[:, ::2]]).contiguous(), 8000, 16000)
    direct = awm.masking(up[:3].contiguous(), up[3:].contiguous())
    assert all(torch.equal(bits(a.float()), bits(b.float())) for a, b in zip(at8, direct))


def test_evaluate_robustness_nmr_columns(awm, dev):
    G, D = reference_models(awm, dev)
    B, T = 3, 16000
    batches = [O.synthetic_clips(B, seed=71, T=T)]
    messages = [torch.tensor([3, 60001, 77])]

    def attacks():
        return {"noise": awm.Distortion(gain_db=0, snr_db=10), "quiet": awm.Distortion(gain_db=0, snr_db=40)}
    old = awm.evaluate_robustness(G, D, batches, attacks(), device=dev, messages=messages, quality=("stoi",))
    res = awm.evaluate_robustness(G, D, batches, attacks(), device=dev, messages=messages, quality=("stoi", "nmr"))
    print(res)
    new = ["audible_share", "audible_share_attack_only", "nmr_db", "nmr_db_attack_only", "nmr_rows"]
    assert list(res) == list(old) == ["none", "noise", "quiet"]
    for name in res:
        assert sorted(res[name]) == sorted(list(old[name]) + new)
        for k in old[name]:
            assert res[name][k] == old[name][k], "the old columns are the old numbers"
    s = batches[0].to(dev)
    G.eval()
    with torch.no_grad():
        delta = awm.postprocess(G(s, messages[0].to(dev)))
    both, ref2 = torch.cat([s + delta, s], dim=0), torch.cat([s, s], dim=0)
    for name, attacked in (("none", both), ("noise", attacks()["noise"](both)), ("quiet", attacks()["quiet"](both))):
        m = awm.masking(ref2, attacked)
        assert m.cells.tolist() == [22 * 61] * (2 * B) and res[name]["nmr_rows"] == B
        assert res[name]["nmr_db"] == float(m.nmr_db[:B].double().mean()), "bit for bit a direct masking call on the same tensors"
        assert res[name]["nmr_db_attack_only"] == float(m.nmr_db[B:].double().mean())
        assert res[name]["audible_share"] == int(m.audible[:B].sum()) / (22 * 61 * B)
        assert res[name]["audible_share_attack_only"] == int(m.audible[B:].sum()) / (22 * 61 * B)
    assert res["none"]["nmr_db_attack_only"] == -math.inf and res["none"]["audible_share_attack_only"] == 0.0, "s against s"
    assert res["noise"]["nmr_db_attack_only"] > res["quiet"]["nmr_db_attack_only"] > -math.inf
    per = awm.evaluate_robustness_by_class(G, D, batches, attacks(), device=dev, messages=messages, quality=("nmr",))
    assert sum(c["nmr_rows"] for c in per["noise"]["by_class"].values()) == B and per["noise"]["nmr_db"] == res["noise"]["nmr_db"]


def test_file_level_nmr(awm, dev):
    G, D = reference_models(awm, dev)
    n = 51200                                            # 3.2 s at 16 kHz: three whole segments and a remainder
    wave = O.synthetic_clips(4, seed=81, T=16000).reshape(1, -1)[:, :n].contiguous()
    torch.manual_seed(5)
    res = awm.generate_watermarked_audio(wave, G, device=dev, nmr=True)
    torch.manual_seed(5)
    plain = awm.generate_watermarked_audio(wave, G, device=dev)
    assert sorted(plain["metrics"]) == ["power_ratio_db", "si_snr_db", "watermark_rms"]
    assert sorted(res["metrics"]) == sorted(list(plain["metrics"]) + ["nmr_db", "audible_share"])
    assert torch.equal(plain["watermarked_waveform"], res["watermarked_waveform"]) and all(plain["metrics"][k] == res["metrics"][k] for k in plain["metrics"])
    m = awm.masking(res["original_waveform"].to(dev), res["watermarked_waveform"].to(dev))
    assert m.cells.tolist() == [22 * Y.frame_count(n)], "the recording is one row"
    assert res["metrics"]["nmr_db"] == float(m.nmr_db[0]) and math.isfinite(res["metrics"]["nmr_db"])
    assert res["metrics"]["audible_share"] == int(m.audible[0]) / int(m.cells[0])
    msgs = torch.tensor([1, 2, 3, 4])
    five = awm.evaluate_unseen_file(wave, G, D, device=dev, messages=msgs, nmr=True)
    six = awm.evaluate_unseen_file(wave, G, D, device=dev, messages=msgs, stoi=True, nmr=True)
    four = awm.evaluate_unseen_file(wave, G, D, device=dev, messages=msgs)
    assert len(four) == 4 and len(five) == 5 and len(six) == 6 and five[4] == six[5] and math.isfinite(five[4])
    assert all(a == b or (a != a and b != b) for a, b in zip(four, five[:4]))
    with torch.no_grad():
        segs = torch.nn.functional.pad(wave, (0, 64000 - n)).reshape(4, 1, 16000).to(dev)
        G.eval()
        wm = (segs + G(segs, msgs.to(dev))).reshape(1, -1)[:, :n]
    assert five[4] == float(awm.masking(wave.to(dev), wm.contiguous()).nmr_db[0])


def test_train_step_with_and_without_the_term(awm, dev):
    G0, D0 = (m.train() for m in reference_models(awm, dev))
    s = O.synthetic_clips(2, seed=41, T=2048).to(dev)
    msg = torch.tensor([3, 60001], device=dev)
    runs = {}
    for name, kw in (("plain", {}), ("none", {"masking": None}), ("term", {"masking": 0.5})):
        G, D = copy.deepcopy(G0), copy.deepcopy(D0)
        opt = torch.optim.Adam(list(G.parameters()) + list(D.parameters()), lr=1e-3)
        out = awm.train_step(G, D, opt, s, msg, **kw)
        runs[name] = (out, [p.grad.clone() for m in (G, D) for p in m.parameters()])
    plain, none, term = runs["plain"], runs["none"], runs["term"]
    assert "mask" not in plain[0] and "mask" not in none[0] and list(plain[0]) == list(none[0])
    assert torch.equal(bits(plain[0]["total"].detach().reshape(1)), bits(none[0]["total"].detach().reshape(1)))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(plain[1], none[1])), "masking=None is the call as it was, bit for bit"
    out = term[0]
    assert math.isfinite(float(out["mask"].detach())) and float(out["mask"].detach()) >= 0.0 and math.isfinite(float(out["total"].detach()))
    assert torch.equal(out["raw_total"], plain[0]["raw_total"]), "raw_total does not see the term"
    want = plain[0]["total"].detach() + 0.5 * out["mask"].detach()
    assert torch.equal(bits(out["total"].detach().reshape(1)), bits(want.reshape(1)))
    direct = awm.masking(s, out["s_w"].detach())
    assert torch.equal(bits(out["mask"].detach().reshape(1)), bits(direct.over_db.mean().reshape(1)))
    print(f"train step: mask {float(out['mask'].detach()):.5f} dB over, nmr {direct.nmr_db.tolist()}")


# ------------------------------------------------------------------------------------------ 6. refusals
def test_bad_arguments(awm, dev):
    st = torch.cuda.current_stream().cuda_stream
    rows, n = 3, 2000
    frames, _, need = M().masking_plan(rows, n)
    x, y, gy = torch.zeros(rows, n, device=dev), torch.zeros(rows, n, device=dev), torch.zeros(rows, n, device=dev)
    nmr, over, gout = torch.zeros(rows, device=dev), torch.zeros(rows, device=dev), torch.ones(rows, device=dev)
    counts = torch.zeros(rows, 2, dtype=torch.int32, device=dev)
    coef = torch.zeros(rows, frames, 22, device=dev)
    sc = torch.zeros(need // 4, dtype=torch.int32, device=dev)
    tab = M().masking_tables()["packed"].to(dev)
    px, py, pt, pn, po, pc, pk, ps, pg, pgy = (t.data_ptr() for t in (x, y, tab, nmr, over, counts, coef, sc, gout, gy))
    ok = (px, py, pt, pn, po, pc, pk, ps, rows, n, st)
    awm.lib.wm_masking_fwd(*ok)
    awm.lib.wm_masking_fwd(px, py, pt, pn, po, pc, None, ps, rows, n, st)          # coef is optional
    for i, v in ((8, 0), (9, 0), (9, 2 ** 34 + 1), (0, None), (2, None), (3, None), (7, None), (0, px + 2), (4, po + 1), (6, pk + 2),
                 (3, px), (7, py), (6, px), (4, pn), (5, pt)):
        args = list(ok)
        args[i] = v
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm.lib.wm_masking_fwd(*args)
    okb = (px, py, pk, pg, pgy, rows, n, st)
    awm.lib.wm_masking_bwd(*okb)
    for i, v in ((5, 0), (6, 0), (0, None), (2, None), (3, None), (4, None), (4, pgy + 2), (1, py + 1), (4, px), (4, py), (4, pk), (4, pg)):
        args = list(okb)
        args[i] = v
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm.lib.wm_masking_bwd(*args)
    with pytest.raises(ValueError):
        awm.masking(x, y[:, :-1])
    with pytest.raises(ValueError):
        awm.masking(x, y.cpu())
    torch.cuda.synchronize()
    assert not gy.any() and not bool(torch.isnan(over).any())
