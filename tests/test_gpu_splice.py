"""The splice attack and the localisation kernels on the GPU (csrc/splice.hip): wm_splice / wm_splice_bwd, wm_bce_masked_fwd / _bwd and
wm_loc_score through the C boundary and through ops, attacks.Splice in a train step, evaluate_localization and locate_watermark.

Everything that selects or counts is compared bit for bit with tests/splice_yardstick.py (integer / float64 numpy, nothing from the
package).  The two masked losses are sums of fp32 terms and are held to float64 by the project's existing rules:
  all labels 1   |masked - fp64| <= 2 |wm_bce_fwd - fp64| + one fp32 ulp of the value (the rule of tests/test_gpu_tail_in_head.py), and
                 dlogits equal to wm_bce_bwd's bit for bit
  any mask       loc, bce within relative 1e-5 of float64, gradients within 1e-4 of the float64 gradient's maximum (the tolerances of
                 wm_bce_* in tests/test_gpu_parity.py); N1 exact; N1 = 0 gives bce == 0.0 and zero bit gradients."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import splice_yardstick as Y
from gpu_support import awm, dev  # noqa: F401
from gpu_support import _spy, p, reference_models, st
from oracle import wm_oracle as O

pytestmark = pytest.mark.gpu

LENGTHS = [1, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4099, 16000]
SEED, DRAW, ROW0 = (7 << 32) + 1, 1, 5
CUT = dict(max_spans=2, p_span=0.5, len_lo=800, len_hi=6400, p_original=1 / 3, p_silence=1 / 3)
FP32_ULP = 2.0 ** -23
SENTINEL = 0x55555555


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def off_by_one_float(a, dev, dtype=np.float32):
    """the same values in a buffer that starts 4 bytes earlier: the returned tensor's pointer is 4 (mod 8)"""
    a = np.ascontiguousarray(a, dtype=dtype)
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a[:0]).dtype, device=dev)
    buf[1:] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[1:].view(a.shape)


def words(n):
    return (n + 31) // 32


def cuts(n):
    """the default cut with its lengths held to the row, and a dense one that has spans of every kind at every n"""
    out = []
    for c in (CUT, dict(max_spans=8, p_span=0.75, len_lo=1, len_hi=max(1, n // 5), p_original=0.25, p_silence=0.25),
              dict(max_spans=3, p_span=1.0, len_lo=max(1, n // 3), len_hi=max(1, n // 2), p_original=0.0, p_silence=0.0)):
        c = dict(c)
        c["len_hi"] = min(c["len_hi"], n)
        c["len_lo"] = min(c["len_lo"], c["len_hi"])
        out.append(c)
    return out


def signals(rows, n, seed=0):
    rng = np.random.default_rng(1000 * seed + n)
    a, b = rng.standard_normal((rows, n)).astype(np.float32), rng.standard_normal((rows, n)).astype(np.float32)
    a[0, 0], b[-1, -1] = -0.0, -0.0
    return a, b


def raw_splice(lib, dev, a, b, cut, seed=SEED, draw=DRAW, row0=ROW0, offset=True):
    """one wm_splice launch on buffers 4 bytes off a 16-byte boundary (offset) or on it; y and lab are filled with sentinels first"""
    rows, n = a.shape
    put = (lambda v, dt=np.float32: off_by_one_float(v, dev, dt)) if offset else (lambda v, dt=np.float32: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).to(dev))
    ad, bd = put(a), put(b)
    y = put(np.full((rows, n), np.nan, dtype=np.float32))
    lab = put(np.full((rows, words(n)), SENTINEL, dtype=np.int32), np.int32)
    if offset:
        assert ad.data_ptr() % 8 == 4 and y.data_ptr() % 8 == 4
    lib.wm_splice(p(ad), p(bd), p(y), p(lab), rows, n, row0, seed, draw, cut["max_spans"], cut["p_span"], cut["len_lo"], cut["len_hi"],
                  cut["p_original"], cut["p_silence"], st())
    return y.cpu().numpy(), lab.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------ 1. wm_splice against the yardstick
@pytest.mark.parametrize("offset", [True, False])
def test_splice_vs_yardstick(awm, dev, offset):
    kinds_seen, covered = set(), 0
    for n in LENGTHS:
        a, b = signals(3, n)
        for cut in cuts(n):
            y, lab = raw_splice(awm.lib, dev, a, b, cut, offset=offset)
            y0, lab0 = Y.splice(a, b, SEED, DRAW, ROW0, **cut)
            assert np.array_equal(lab, Y.pack(lab0)), f"n={n} {cut}: labels (tail bits included)"
            assert np.array_equal(bits(y), bits(y0)), f"n={n} {cut}: samples"
            covered += int((~lab0).sum())
            kinds_seen |= {s[2] for r in range(3) for s in Y.spans(SEED, DRAW, ROW0 + r, n, **cut) if s[4]}
    assert kinds_seen == {0, 1, 2} and covered > 1000, "the cases must exercise every kind"


def test_splice_rows_draws_and_determinism(awm, dev):
    for n in (33, 257, 4099, 16000):
        a, b = signals(3, n, seed=1)
        cut = cuts(n)[1]
        y, lab = raw_splice(awm.lib, dev, a, b, cut)
        y2, lab2 = raw_splice(awm.lib, dev, a, b, cut)
        assert np.array_equal(bits(y), bits(y2)) and np.array_equal(lab, lab2), "two launches"
        for r in range(3):
            yr, lr = raw_splice(awm.lib, dev, a[r:r + 1], b[r:r + 1], cut, row0=ROW0 + r)
            assert np.array_equal(bits(yr), bits(y[r:r + 1])) and np.array_equal(lr, lab[r:r + 1]), f"n={n}: row {r} alone"
        y3, lab3 = raw_splice(awm.lib, dev, a, b, cut, draw=DRAW + 1)
        y4, lab4 = raw_splice(awm.lib, dev, a, b, cut, seed=SEED + (1 << 32))
        assert not np.array_equal(lab3, lab) and not np.array_equal(lab4, lab), "the draw and the seed's high word count"


def test_splice_8_row_fixture_and_conventions(awm, dev):
    """the CPU suite's 8-row fixture (a row without a span, a row with two overlapping spans, all three kinds) through the module"""
    from awm_amd import attacks as A
    n = 16000
    a, b = signals(8, n, seed=2)
    rows = [Y.spans(SEED, DRAW, ROW0 + r, n, **CUT) for r in range(8)]
    assert any(not any(s[4] for s in row) for row in rows)
    assert any(all(s[4] for s in row) and row[0][0] < row[1][0] + row[1][1] and row[1][0] < row[0][0] + row[0][1] for row in rows)
    assert {s[2] for row in rows for s in row if s[4]} == {0, 1, 2}
    sp = A.Splice(seed=SEED).reset(DRAW)
    y, lab = sp(torch.from_numpy(a).to(dev).view(8, 1, n), torch.from_numpy(b).to(dev).view(8, 1, n), row0=ROW0)
    y0, lab0 = Y.splice(a, b, SEED, DRAW, ROW0, **CUT)
    assert y.shape == (8, 1, n) and lab.dtype == torch.int32 and tuple(lab.shape) == (8, 500)
    assert np.array_equal(bits(y.cpu().numpy().reshape(8, n)), bits(y0)) and np.array_equal(lab.cpu().numpy().view(np.uint32), Y.pack(lab0))
    yc, labc = sp.reset(DRAW)(torch.from_numpy(a).view(8, 1, n), torch.from_numpy(b).view(8, 1, n), row0=ROW0)
    assert torch.equal(yc, y.cpu()) and torch.equal(labc, lab.cpu()), "the CPU restatement and the kernel agree bit for bit"
    # p_span = 0: y = a and all labels 1; len_lo = len_hi = n: every label 0
    y, lab = raw_splice(awm.lib, dev, a, b, dict(CUT, p_span=0.0))
    assert np.array_equal(bits(y), bits(a)) and np.array_equal(lab, Y.pack(np.ones((8, n), bool)))
    y, lab = raw_splice(awm.lib, dev, a, b, dict(CUT, p_span=1.0, len_lo=n, len_hi=n, p_original=1.0, p_silence=0.0))
    assert np.array_equal(bits(y), bits(b)) and not lab.any()


def test_splice_refusals_launch_nothing(awm, dev):
    lib = awm.lib
    n, rows = 100, 2
    a = torch.randn(rows * n + 8, device=dev)
    b = torch.randn(rows * n + 8, device=dev)
    y = torch.full((rows * n + 8,), 7.0, device=dev)
    lab = torch.full((rows * words(n) + 8,), SENTINEL, dtype=torch.int32, device=dev)
    ok = dict(a=p(a), b=p(b), y=p(y), lab=p(lab), rows=rows, n=n, row0=0, seed=1, draw=0, max_spans=2, p_span=1.0, len_lo=10, len_hi=50,
              p_original=0.25, p_silence=0.25)

    def call(**kw):
        v = dict(ok, **kw)
        lib.wm_splice(v["a"], v["b"], v["y"], v["lab"], v["rows"], v["n"], v["row0"], v["seed"], v["draw"], v["max_spans"], v["p_span"],
                      v["len_lo"], v["len_hi"], v["p_original"], v["p_silence"], st())

    bad = [dict(y=p(a)), dict(y=p(b)), dict(y=p(a) + 4 * n), dict(lab=p(a)), dict(lab=p(y)), dict(a=None), dict(b=None), dict(y=None),
           dict(lab=None), dict(a=p(a) + 2), dict(y=p(y) + 2), dict(lab=p(lab) + 1), dict(rows=0), dict(n=0), dict(n=2 ** 24 + 1, len_hi=50),
           dict(row0=-1), dict(row0=2 ** 32 - 1), dict(draw=-1), dict(draw=2 ** 32), dict(max_spans=0), dict(max_spans=9), dict(len_lo=0),
           dict(len_lo=51), dict(len_hi=n + 1), dict(p_span=-0.5), dict(p_span=1.5), dict(p_span=math.nan), dict(p_original=math.nan),
           dict(p_original=0.75, p_silence=0.5), dict(p_silence=-0.25)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="wm_splice failed"):
            call(**kw)
    da = torch.full((rows * n + 8,), 7.0, device=dev)
    for args in ((p(a), p(lab), p(a), rows, n), (p(a), p(lab), p(lab), rows, n), (None, p(lab), p(da), rows, n), (p(a), None, p(da), rows, n),
                 (p(a), p(lab), None, rows, n), (p(a), p(lab), p(da) + 2, rows, n), (p(a), p(lab), p(da), 0, n), (p(a), p(lab), p(da), rows, 0),
                 (p(a), p(lab), p(da), rows, 2 ** 24 + 1)):
        with pytest.raises(RuntimeError, match="wm_splice_bwd failed"):
            lib.wm_splice_bwd(*args, st())
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((da == 7.0).all()) and bool((lab == SENTINEL).all()), "a refused call writes nothing"
    call()                                                             # and the arguments they were derived from are accepted
    assert bool((lab[:rows * words(n)] != SENTINEL).all()) and bool((lab[rows * words(n):] == SENTINEL).all())


# ------------------------------------------------------------------------------------------ 2. wm_splice_bwd, autograd
def test_splice_bwd_is_where_label(awm, dev):
    for n in LENGTHS:
        rng = np.random.default_rng(n)
        labels = rng.random((3, n)) < 0.6
        dy = rng.standard_normal((3, n)).astype(np.float32)
        dy[0, 0], dy[1, n // 2], dy[2, -1] = -0.0, np.nan, np.inf
        for offset in (True, False):
            put = (lambda v, dt: off_by_one_float(v, dev, dt)) if offset else (lambda v, dt: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).to(dev))
            dyd, labd = put(dy, np.float32), put(Y.pack(labels).view(np.int32), np.int32)
            da = put(np.full((3, n), np.nan), np.float32)
            awm.lib.wm_splice_bwd(p(dyd), p(labd), p(da), 3, n, st())
            want = np.where(labels, dy, np.float32(0.0))
            assert np.array_equal(bits(da.cpu().numpy()), bits(want)), f"n={n} offset={offset}"


def test_splice_autograd(awm, dev):
    from awm_amd import attacks as A, ops
    n = 4099
    a, b = signals(3, n, seed=3)
    ta = torch.from_numpy(a).to(dev).requires_grad_(True)
    tb = torch.from_numpy(b).to(dev).requires_grad_(True)
    cut = cuts(n)[1]
    y, lab = ops.splice(ta, tb, seed=SEED, draw=DRAW, row0=ROW0, **cut)
    assert y.requires_grad and not lab.requires_grad and lab.dtype == torch.int32
    dy = torch.randn(3, n, device=dev)
    y.backward(dy)
    labels = torch.from_numpy(A.unpack_labels(lab, n)).to(dev)
    assert 0 < float(labels.float().mean()) < 1
    assert torch.equal(ta.grad, torch.where(labels, dy, torch.zeros_like(dy))), "the gradient is dy where the label is 1"
    assert tb.grad is None, "b is data"
    with pytest.raises(RuntimeError):
        ops.splice(ta.detach().cpu(), tb.detach().cpu(), **cut)         # no CPU fallback below the module


# ------------------------------------------------------------------------------------------ 3. the masked losses
def _logits(R, T, NO, dev, seed=0):
    g = torch.Generator().manual_seed(100 * R + 10 * NO + T + seed)
    return (3.0 * torch.randn(R, T, NO, generator=g)).to(dev)


def _messages(B, NO, dev):
    g = torch.Generator().manual_seed(7 + NO)
    return torch.randint(0, 1 << max(NO - 1, 1), (B,), generator=g, dtype=torch.int64).to(dev)


def masked_fwd(lib, logits, msg, lab):
    R, T, NO = logits.shape
    B = msg.shape[0]
    part = torch.empty(3 * R * ((T * NO + 4095) // 4096), device=logits.device)
    out = torch.full((2,), -7.0, device=logits.device)
    count = torch.full((1,), -1, dtype=torch.int64, device=logits.device)
    lib.wm_bce_masked_fwd(p(logits), p(msg), p(lab), p(part), p(count), p(out[0]), p(out[1]), B, R, T, NO, st())
    return float(out[0]), float(out[1]), int(count), count


def masked_bwd(lib, logits, msg, lab, count, g_loc, g_bce):
    R, T, NO = logits.shape
    gl, gb = torch.tensor([g_loc], device=logits.device), torch.tensor([g_bce], device=logits.device)
    d = torch.full_like(logits, float("nan"))
    lib.wm_bce_masked_bwd(p(logits), p(msg), p(lab), p(count), p(gl), p(gb), p(d), msg.shape[0], R, T, NO, st())
    return d


@pytest.mark.parametrize("NO", [1, 2, 17])
@pytest.mark.parametrize("B", [1, 3])
def test_masked_losses_with_all_labels_one(awm, dev, B, NO):
    lib = awm.lib
    for T in (33, 257, 1000):
        R = 2 * B
        logits, msg = _logits(R, T, NO, dev), _messages(B, NO, dev)
        labels = np.ones((B, T), dtype=bool)
        lab = off_by_one_float(Y.pack(labels).view(np.int32), dev, np.int32)
        part = torch.empty(2 * R * ((T * NO + 4095) // 4096), device=dev)
        ref = torch.full((2,), -7.0, device=dev)
        lib.wm_bce_fwd(p(logits), p(msg), p(part), p(ref[0]), p(ref[1]), B, R, T, NO, st())
        loc, bce, n1, count = masked_fwd(lib, logits, msg, lab)
        loc64, bce64, n64, dloc, dbce = Y.masked_losses(logits.cpu().numpy(), msg.cpu().numpy(), labels, B)
        assert n1 == n64 == B * T
        for name, got, unmasked, want in (("loc", loc, float(ref[0]), loc64), ("bce", bce, float(ref[1]), bce64)):
            if want is None:
                assert got == -7.0 and unmasked == -7.0, "NO = 1 leaves bce_out untouched"
                continue
            e_m, e_u = abs(got - want), abs(unmasked - want)
            print(f"B={B} NO={NO} T={T} {name}: masked {e_m:.3e} unmasked {e_u:.3e} from fp64 ({want:.6f})")
            assert e_m <= 2.0 * e_u + FP32_ULP * abs(want), f"{name}: masked {e_m:.3e} unmasked {e_u:.3e}"
        gl, gb = torch.tensor([10.0], device=dev), torch.tensor([1.0], device=dev)
        d_ref = torch.full_like(logits, float("nan"))
        lib.wm_bce_bwd(p(logits), p(msg), p(gl), p(gb), p(d_ref), B, R, T, NO, st())
        d = masked_bwd(lib, logits, msg, lab, count, 10.0, 1.0)
        assert torch.equal(d.view(torch.int32), d_ref.view(torch.int32)), "with every label 1 dlogits is wm_bce_bwd's, bit for bit"


def _masks(B, T, rng, awm, dev):
    """name -> bool (B, T): drawn by the kernel, drawn at random, and the hand-made ones"""
    cut = dict(max_spans=3, p_span=0.9, len_lo=max(1, T // 8), len_hi=max(1, T // 3), p_original=1 / 3, p_silence=1 / 3)
    z = np.zeros((B, T), dtype=np.float32)
    _, lab = raw_splice(awm.lib, dev, z, z, cut, offset=False)
    single = np.zeros((B, T), dtype=bool)
    single[B - 1, T // 2] = True
    tail = np.zeros((B, T), dtype=bool)
    tail[:, 32 * ((T - 1) // 32):] = True                              # the last (partial, T % 32 != 0) word only
    return {"splice": Y.unpack(lab, T), "random": rng.random((B, T)) < 0.5, "all_zero": np.zeros((B, T), dtype=bool), "single_bit": single,
            "last_word": tail}


@pytest.mark.parametrize("NO", [1, 2, 17])
@pytest.mark.parametrize("B", [1, 3])
def test_masked_losses_vs_float64(awm, dev, B, NO):
    lib = awm.lib
    for T in (33, 257, 1000):
        R = 2 * B
        logits, msg = _logits(R, T, NO, dev, seed=1), _messages(B, NO, dev)
        for name, labels in _masks(B, T, np.random.default_rng(T + NO), awm, dev).items():
            lab = off_by_one_float(Y.pack(labels).view(np.int32), dev, np.int32)
            loc, bce, n1, count = masked_fwd(lib, logits, msg, lab)
            loc64, bce64, n64, dloc, dbce = Y.masked_losses(logits.cpu().numpy(), msg.cpu().numpy(), labels, B)
            what = f"B={B} NO={NO} T={T} {name}"
            assert n1 == n64, f"{what}: N1 {n1} vs {n64}"
            print(f"{what}: N1 {n1} loc {loc:.7f} ({loc64:.7f}) bce {bce:.7f} ({bce64})")
            assert abs(loc - loc64) <= 1e-5 * abs(loc64), f"{what}: loc {loc!r} vs {loc64!r}"
            if NO > 1:
                assert abs(bce - bce64) <= 1e-5 * abs(bce64), f"{what}: bce {bce!r} vs {bce64!r}"
                if n1 == 0:
                    assert bce == 0.0
            else:
                assert bce == -7.0, "NO = 1 leaves bce_out untouched"
            loc_b, bce_b, _, _ = masked_fwd(lib, logits, msg, lab)
            assert (loc_b, bce_b) == (loc, bce), "two launches give the same bits"
            d = masked_bwd(lib, logits, msg, lab, count, 10.0, 1.0).double().cpu().numpy()
            d64 = 10.0 * dloc + 1.0 * dbce
            err = np.abs(d - d64).max()
            print(f"{what}: gradient max err {err:.3e} of max {np.abs(d64).max():.3e}")
            assert err <= 1e-4 * np.abs(d64).max(), f"{what}: gradient"
            if NO > 1:
                gate = np.zeros((R, T), dtype=bool)
                gate[:B] = labels
                assert not d[:, :, 1:][~gate].any(), f"{what}: bit gradients outside the labels must be zero"
                if n1 == 0:
                    assert not d[:, :, 1:].any()


def test_masked_bce_fn_and_refusals(awm, dev):
    from awm_amd import losses as L, ops
    B, T, NO = 2, 257, 17
    logits = _logits(2 * B, T, NO, dev, seed=2).requires_grad_(True)
    msg = _messages(B, NO, dev)
    labels = np.random.default_rng(5).random((B, T)) < 0.7
    lab = torch.from_numpy(Y.pack(labels).view(np.int32)).to(dev)
    loc, bce = L.detection_losses_masked(logits, msg, lab)
    (10.0 * loc + bce).backward()
    loc64, bce64, _, dloc, dbce = Y.masked_losses(logits.detach().cpu().numpy(), msg.cpu().numpy(), labels, B)
    assert abs(float(loc.detach()) - loc64) <= 1e-5 * loc64 and abs(float(bce.detach()) - bce64) <= 1e-5 * bce64
    d64 = 10.0 * dloc + dbce
    assert np.abs(logits.grad.double().cpu().numpy() - d64).max() <= 1e-4 * np.abs(d64).max()
    with pytest.raises(ValueError):
        ops.MaskedBCEFn.apply(logits, msg, lab[:, :-1])
    with pytest.raises(ValueError):
        ops.MaskedBCEFn.apply(logits, msg, lab.to(torch.int64))
    with pytest.raises(ValueError):
        ops.MaskedBCEFn.apply(logits[:3], msg, lab)
    lg = logits.detach()
    part, out, cnt = torch.empty(64, device=dev), torch.zeros(2, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    for args in ((None, p(msg), p(lab), p(part), p(cnt), p(out[0]), p(out[1]), B, 2 * B, T, NO),
                 (p(lg), None, p(lab), p(part), p(cnt), p(out[0]), p(out[1]), B, 2 * B, T, NO),
                 (p(lg), p(msg), None, p(part), p(cnt), p(out[0]), p(out[1]), B, 2 * B, T, NO),
                 (p(lg), p(msg), p(lab), p(part), None, p(out[0]), p(out[1]), B, 2 * B, T, NO),
                 (p(lg), p(msg), p(lab), p(part), p(cnt), p(out[0]), None, B, 2 * B, T, NO),
                 (p(lg), p(msg), p(lab), p(part), p(cnt), p(out[0]), p(out[1]), 2 * B + 1, 2 * B, T, NO),
                 (p(lg), p(msg), p(lab), p(part), p(cnt), p(out[0]), p(out[1]), B, 0, T, NO),
                 (p(lg), p(msg), p(lab), p(part), p(cnt), p(out[0]), p(out[1]), B, 2 * B, 2 ** 20, NO)):
        with pytest.raises(RuntimeError, match="wm_bce_masked_fwd failed"):
            awm.lib.wm_bce_masked_fwd(*args, st())
    g = torch.ones(1, device=dev)
    with pytest.raises(RuntimeError, match="wm_bce_masked_bwd failed"):
        awm.lib.wm_bce_masked_bwd(p(lg), p(msg), p(lab), p(cnt), p(g), p(g), p(lg), B, 2 * B, T, NO, st())     # in place


# ------------------------------------------------------------------------------------------ 4. wm_loc_score
@pytest.mark.parametrize("NO", [1, 17])
def test_loc_score_counts_and_pred(awm, dev, NO):
    from awm_amd import ops
    R = 3
    for T in LENGTHS:
        for thr_p in (0.5, 0.7):
            thr = ops.loc_threshold_logit(thr_p)
            x = _logits(R, T, NO, dev, seed=3).cpu().numpy()
            special = [np.float32(thr), np.nextafter(np.float32(thr), np.float32(np.inf)), 0.0, -0.0, np.nan, np.inf, -np.inf]
            for i, v in enumerate(special):
                if i < T:
                    x[i % R, (5 * i) % T, 0] = v
            x[:, :, 1:] = np.where(x[:, :, 1:] > 0, 50.0, -50.0) if NO > 1 else x[:, :, 1:]      # the other channels must not matter
            labels = np.random.default_rng(T).random((R, T)) < 0.5
            xd = off_by_one_float(x, dev)
            for lab_rows in (R, 1, None):
                lab = None if lab_rows is None else off_by_one_float(Y.pack(labels[:lab_rows]).view(np.int32), dev, np.int32)
                counts = off_by_one_float(np.full((R, 4), -1), dev, np.int32)
                pred = off_by_one_float(np.full((R, words(T)), SENTINEL), dev, np.int32)
                awm.lib.wm_loc_score(p(xd), p(lab), float(thr), p(counts), p(pred), R, T, NO, lab_rows or 0, st())
                c0, pred0 = Y.loc_counts(x, None if lab_rows is None else labels[:lab_rows], thr, lab_rows)
                what = f"NO={NO} T={T} thr={thr_p} lab_rows={lab_rows}"
                assert np.array_equal(counts.cpu().numpy(), c0), f"{what}: counts"
                assert np.array_equal(pred.cpu().numpy().view(np.uint32), Y.pack(pred0)), f"{what}: pred (tail bits zero)"
                assert (c0.sum(axis=1) == T).all()
                counts2 = torch.full((R, 4), -1, dtype=torch.int32, device=dev)
                awm.lib.wm_loc_score(p(xd), p(lab), float(thr), p(counts2), None, R, T, NO, lab_rows or 0, st())
                assert np.array_equal(counts2.cpu().numpy(), c0), f"{what}: counts without pred"
    # through ops
    x = _logits(4, 257, NO, dev, seed=4)
    labels = np.random.default_rng(1).random((2, 257)) < 0.5
    lab = torch.from_numpy(Y.pack(labels).view(np.int32)).to(dev)
    counts, pred = ops.loc_counts(x, lab, 0.5, want_pred=True)
    c0, pred0 = Y.loc_counts(x.cpu().numpy(), labels, 0.0, 2)
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), c0) and np.array_equal(pred.cpu().numpy().view(np.uint32), Y.pack(pred0))
    assert torch.equal(ops.loc_counts(x, lab), counts)
    for args in ((None, p(lab), 0.0, p(counts), None, 4, 257, NO, 2), (p(x), p(lab), 0.0, None, None, 4, 257, NO, 2),
                 (p(x), p(lab), math.nan, p(counts), None, 4, 257, NO, 2), (p(x), p(lab), 0.0, p(counts), None, 4, 257, NO, 5),
                 (p(x), p(lab), 0.0, p(counts), None, 0, 257, NO, 0), (p(x), p(lab), 0.0, p(counts), None, 4, 0, NO, 2)):
        with pytest.raises(RuntimeError, match="wm_loc_score failed"):
            awm.lib.wm_loc_score(*args, st())


# ------------------------------------------------------------------------------------------ 5. end to end, main16 models at B = 2
NET_B, NET_T = 2, 2048           # the shortest clip the step's loudness loss accepts
SPIED = ("wm_splice", "wm_splice_bwd", "wm_bce_masked_fwd", "wm_bce_masked_bwd", "wm_bce_fwd", "wm_bce_bwd", "wm_headN_tail_fwd",
         "wm_headN_bwd_bce", "wm_headN_fwd", "wm_headN_bwd", "wm_loc_score")


def _golden_detector(awm, dev):
    ck = np.load(os.path.join(os.path.dirname(__file__), "golden", "detector_best_unprefixed.npz"))
    D = awm.Detector(16)
    D.load_state_dict({k: torch.from_numpy(ck[k]) for k in ck.files})
    return D.to(dev)


def test_train_step_with_and_without_tamper(awm, dev, monkeypatch):
    G0, D0 = (m.train() for m in reference_models(awm, dev))
    s = O.synthetic_clips(NET_B, seed=41, T=NET_T).to(dev)
    msg = torch.tensor([3, 60001], device=dev)
    runs = {}
    for name, tamper in (("plain", None), ("tamper", awm.Splice(max_spans=3, p_span=1.0, length_s=(0.01, 0.03), seed=SEED).reset(DRAW))):
        G, D = copy.deepcopy(G0), copy.deepcopy(D0)
        opt = torch.optim.Adam(list(G.parameters()) + list(D.parameters()), lr=1e-3)
        before = {k: v.clone() for m in (G, D) for k, v in m.state_dict().items()}
        with monkeypatch.context() as mp:
            counts = _spy(mp, awm.lib, SPIED)
            out = awm.train_step(G, D, opt, s, msg) if tamper is None else awm.train_step(G, D, opt, s, msg, tamper=tamper)
        moved = [not torch.equal(before[k], v) for m in (G, D) for k, v in m.state_dict().items() if v.dtype.is_floating_point]
        runs[name] = (out, counts, moved)
    out, counts, moved = runs["plain"]
    # what the step launches today: the fused Detector tail, no separate BCE pass, nothing of this file
    assert counts.get("wm_headN_tail_fwd") == 1 and counts.get("wm_headN_bwd_bce") == 1, counts
    assert not any(k in counts for k in ("wm_splice", "wm_splice_bwd", "wm_bce_masked_fwd", "wm_bce_masked_bwd", "wm_bce_fwd", "wm_loc_score")), counts
    assert "labels" not in out and "s_t" not in out and all(moved)
    out_t, counts, moved = runs["tamper"]
    assert counts.get("wm_splice") == 1 and counts.get("wm_splice_bwd") == 1, counts
    assert counts.get("wm_bce_masked_fwd") == 1 and counts.get("wm_bce_masked_bwd") == 1, counts
    assert "wm_headN_bwd_bce" not in counts and "wm_headN_tail_fwd" not in counts and "wm_bce_fwd" not in counts, counts
    assert all(moved), "every parameter moves"
    # the splice is the yardstick's on the step's own s_w; mel, loudness, l1 and hf saw the unspliced signals
    cut = dict(max_spans=3, p_span=1.0, len_lo=160, len_hi=480, p_original=np.float32(1 / 3), p_silence=np.float32(1 / 3))
    y0, lab0 = Y.splice(out_t["s_w"].detach().cpu().numpy().reshape(NET_B, NET_T), s.cpu().numpy().reshape(NET_B, NET_T), SEED, DRAW, 0, **cut)
    assert np.array_equal(bits(out_t["s_t"].detach().cpu().numpy().reshape(NET_B, NET_T)), bits(y0))
    assert np.array_equal(out_t["labels"].cpu().numpy().view(np.uint32), Y.pack(lab0)) and 0 < lab0.mean() < 1
    for k in ("delta", "s_w", "l1", "mel", "loud", "hf"):
        assert torch.equal(out_t[k], out[k]), f"{k} must not see the splice"
    loc64, bce64, _, _, _ = Y.masked_losses(out_t["logits"].detach().cpu().numpy(), msg.cpu().numpy(), lab0, NET_B)
    print(f"train step: loc {float(out_t['loc']):.7f} ({loc64:.7f}) bce {float(out_t['bce']):.7f} ({bce64:.7f})")
    assert abs(float(out_t["loc"]) - loc64) <= 1e-5 * loc64 and abs(float(out_t["bce"]) - bce64) <= 1e-5 * bce64
    assert float(out_t["loc"]) != float(out["loc"])


def test_evaluate_localization_equals_host_recomputation(awm, dev):
    D = _golden_detector(awm, dev)
    torch.manual_seed(17)
    G = awm.Generator(16).to(dev)
    batches = [O.synthetic_clips(2, seed=51, T=NET_T), O.synthetic_clips(2, seed=52, T=NET_T)]
    messages = [torch.tensor([3, 60001]), torch.tensor([77, 12345])]
    tamper = awm.Splice(max_spans=2, p_span=1.0, length_s=(0.02, 0.05), seed=9)
    seen = []
    hook = D.register_forward_hook(lambda mod, args, result: seen.append(result.detach().cpu().numpy()))
    try:
        res = awm.evaluate_localization(G, D, batches, tamper, device=dev, messages=messages, threshold=0.5)
    finally:
        hook.remove()
    print(res)
    assert tamper.draw == 2 and len(seen) == 2 and res["rows"] == 4
    pooled, clean, accs = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64), []
    zeros = np.zeros((2, NET_T), dtype=np.float32)
    for bi, logits in enumerate(seen):
        _, labels = Y.splice(zeros, zeros, 9, bi, 0, **{k: (np.float32(v) if k.startswith("p_") else v) for k, v in tamper.cut(NET_T).items()})
        c, _ = Y.loc_counts(logits, labels, 0.0, 2)
        pooled += c[:2].sum(axis=0)
        clean += c[2:].sum(axis=0)
        for r in range(2):
            if labels[r].any():
                votes = (logits[r][labels[r]][:, 1:] > 0).sum(axis=0)
                decoded = 2 * votes > labels[r].sum()
                want = (int(messages[bi][r]) >> np.arange(16)) & 1
                accs.append(np.float32((decoded == want.astype(bool)).mean()))
    tp, fp, fn, tn = (int(v) for v in pooled)
    assert tp + fp + fn + tn == 4 * NET_T and clean[0] == 0 and clean[2] == 0
    nan_or = lambda a, b: a / b if b else math.nan
    want = dict(iou=nan_or(tp, tp + fp + fn), precision=nan_or(tp, tp + fp), recall=nan_or(tp, tp + fn), sample_accuracy=(tp + tn) / (4 * NET_T),
                clean_false_positive_rate=nan_or(int(clean[1]), int(clean[1] + clean[3])), watermarked_fraction=(tp + fn) / (4 * NET_T))
    for k, v in want.items():
        assert res[k] == v or (math.isnan(res[k]) and math.isnan(v)), f"{k}: {res[k]!r} vs {v!r}"
    assert abs(res["bit_accuracy"] - float(np.mean(np.array(accs, dtype=np.float64)))) < 1e-12
    assert 0 < res["watermarked_fraction"] < 1


def _host_runs(pred, min_len):
    """runs of `pred` as (start, end, value), the first of the shortest runs merged into its neighbours while it is shorter than min_len"""
    runs = []
    for t, v in enumerate(pred):
        if runs and runs[-1][2] == bool(v):
            runs[-1][1] = t + 1
        else:
            runs.append([t, t + 1, bool(v)])
    while len(runs) > 1:
        i = min(range(len(runs)), key=lambda k: (runs[k][1] - runs[k][0], k))
        if runs[i][1] - runs[i][0] >= min_len:
            break
        lo, hi = max(i - 1, 0), min(i + 1, len(runs) - 1)
        runs[lo:hi + 1] = [[runs[lo][0], runs[hi][1], not runs[i][2]]]
    return runs


def test_locate_watermark_equals_the_thresholded_track(awm, dev, monkeypatch):
    D = _golden_detector(awm, dev)
    torch.manual_seed(17)
    G = awm.Generator(16).to(dev)
    n = 40000                                                          # 2.5 s: three segments, the last one padded
    original = O.synthetic_clips(3, seed=61, T=16000).reshape(1, -1)[:, :n].contiguous()
    wm, _, _ = awm.embed_waveform(original, G, device=dev, messages=torch.tensor([1, 2, 3]))
    wm[:, 12000:28000] = original[:, 12000:28000]                       # the middle second is clean
    with monkeypatch.context() as mp:
        counts = _spy(mp, awm.lib, ("wm_loc_score",))
        for thr, min_len_s in ((0.5, 0.02), (0.5, 0.0), (0.3, 0.005)):
            res = awm.locate_watermark(wm, D, threshold=thr, min_len_s=min_len_s, device=dev)
            track = awm.detect_waveform(wm, D, device=dev)["temporal_probs"]
            assert track.shape == (n,)
            pred = track > np.float32(thr)
            runs = _host_runs(pred, min_len_s * 16000)
            want = {True: [], False: []}
            for a, b, v in runs:
                want[v].append((a / 16000, b / 16000))
            print(f"thr {thr} min_len {min_len_s}: {len(res['watermarked'])} watermarked, {len(res['unmarked'])} unmarked intervals, "
                  f"fraction {res['fraction_watermarked']:.4f}")
            assert res["watermarked"] == want[True] and res["unmarked"] == want[False]
            assert res["fraction_watermarked"] == float(pred.mean())
            spans = sorted(res["watermarked"] + res["unmarked"])
            assert spans[0][0] == 0.0 and spans[-1][1] == n / 16000 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), "the lists tile the recording"
    assert counts.get("wm_loc_score") == 3, "one launch per call: the track itself never leaves the device"
    empty = awm.locate_watermark(torch.zeros(1, 0), D, device=dev)
    assert empty["watermarked"] == [] and empty["unmarked"] == [] and math.isnan(empty["fraction_watermarked"])
