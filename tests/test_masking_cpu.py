"""The masking model without a GPU: the yardstick of tests/masking_yardstick.py against the definition's own properties, the package's host
restatement (masking.masking_rows_host, MaskingLoss on CPU tensors) against the yardstick, the tables, the C boundary and the wiring."""
import importlib
import inspect
import math
import os

import numpy as np
import pytest
import torch

import masking_yardstick as Y


class _Module:
    """awm_amd.masking is the function; the module of that name is reached through the import system"""
    def __getattr__(self, name):
        return getattr(importlib.import_module("awm_amd.masking"), name)


M = _Module()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "audio-watermarking-deep-learning-watermarks-for-authenticating-speech_amd")


# ------------------------------------------------------------------------------------------ the yardstick against the definition
def test_table_pins():
    t = Y.tables64()
    assert len(t.G) == len(t.A) == 22 and t.S.shape == (22, 22)
    assert int(np.floor(Y.bark(8000.0))) + 1 == 22
    assert np.bincount(t.band).tolist() == list(Y.BIN_COUNTS) and sum(Y.BIN_COUNTS) == 257
    assert (np.diff(t.band) >= 0).all() and t.band[0] == 0 and t.band[-1] == 21
    assert t.c[0] == t.c[256] == (8.0 / 3.0) / 512 ** 2 and (t.c[1:256] == 2.0 * t.c[0]).all()
    assert (t.A > 0).all() and np.allclose(t.G, t.S.sum(axis=1))


def test_full_scale_sine_sums_to_one_half():
    x = np.sin(2.0 * np.pi * 1000.0 * np.arange(2048) / Y.FS)                    # 1 kHz is bin 32: the leakage is the Hann window's two neighbours
    P, _, _ = Y.spectra(x)
    assert P.shape == (7, 257)
    assert np.abs(P.sum(axis=1) - 0.5).max() < 1e-12
    x = np.sin(2.0 * np.pi * 1010.0 * np.arange(2048) / Y.FS)                    # off the grid: to window leakage
    P, _, _ = Y.spectra(x)
    assert np.abs(P.sum(axis=1) - 0.5).max() < 0.01


def test_scaling_the_difference_moves_nmr_by_the_same_db():
    x, y = Y.case(4608)
    x0, d0 = x[1].astype(np.float64), y[1].astype(np.float64) - x[1].astype(np.float64)
    base = Y.model(x0, x0 + d0)
    for a in (-20.0, 6.0, 13.5):
        got = Y.model(x0, x0 + 10.0 ** (a / 20.0) * d0)
        assert abs(got.nmr_db - base.nmr_db - a) < 1e-9, (a, got.nmr_db - base.nmr_db)


def test_silent_reference_leaves_the_threshold_in_quiet():
    T = Y.mask(np.zeros(1280))
    assert T.shape == (4, 22) and (T == Y.tables64().A[None, :]).all()
    T32 = Y.mask(np.zeros(1280, dtype=np.float32), twin=True)
    assert T32.dtype == np.float32 and (T32 == Y.tables(True).A[None, :]).all()


@pytest.mark.parametrize("n", [1280, 4608])
def test_gradient_matches_a_central_difference(n):
    x, y = Y.case(n)
    rng = np.random.default_rng(n)
    checked = 0
    for i in range(3):
        x0, y0 = x[i].astype(np.float64), y[i].astype(np.float64)
        ref = Y.model(x0, y0)
        if not np.any(ref.grad):
            continue
        assert Y.hinge_distance(ref) > Y.HINGE_MARGIN                               # the active set does not move under the probe
        for j in rng.integers(0, n, 6):
            h = 1e-7
            yp, ym = y0.copy(), y0.copy()
            yp[j] += h
            ym[j] -= h
            fd = (Y.model(x0, yp).over_db - Y.model(x0, ym).over_db) / (2.0 * h)
            assert abs(fd - ref.grad[j]) <= 1e-7 * np.abs(ref.grad).max(), (i, j, fd, ref.grad[j])
            checked += 1
    assert checked >= 6
    assert (Y.model(x[2], y[2]).grad[256 * (Y.frame_count(n) + 1):] == 0).all()    # the unjudged tail


def test_float32_mode_stays_float32_and_close():
    r64, r32 = Y.case_ref(4608)
    for a, b in zip(r64, r32):
        assert b.r.dtype == np.float32 and b.grad.dtype == np.float32 and a.r.dtype == np.float64
        assert a.audible == b.audible and a.cells == b.cells == 22 * Y.frame_count(4608)
    fn, fo, fg = Y.floors(4608)
    print(f"float32 floors at n = 4608: nmr {fn:.2e} dB, over {fo:.2e} dB, gradient {fg:.2e}")
    assert 0 < fn < 1e-4 and fo < 1e-5 and 0 < fg < 1e-5


# ------------------------------------------------------------------------------------------ the package's host path
def test_package_tables_are_the_yardsticks_rounded_once():
    tab, t32 = M.masking_tables(), Y.tables(True)
    for k in ("w", "c", "S", "G", "A"):
        assert tab[k].dtype == torch.float32 and np.array_equal(tab[k].numpy(), getattr(t32, k)), k
    assert tab["band"].dtype == torch.int32 and np.array_equal(tab["band"].numpy(), t32.band)
    packed = tab["packed"]
    assert packed.dtype == torch.float32 and packed.numel() == 257 + 257 + 484 + 22 + 22 == 1042
    assert torch.equal(packed[:257], tab["c"]) and torch.equal(packed[257:514].view(torch.int32), tab["band"])
    assert torch.equal(packed[514:998], tab["S"].reshape(-1)) and torch.equal(packed[998:1020], tab["G"]) and torch.equal(packed[1020:], tab["A"])


@pytest.mark.parametrize("n", [767, 4608])
def test_host_rows_and_loss_match_the_yardstick(n):
    import awm_amd
    x, y = Y.case(n)
    r64, _ = Y.case_ref(n)
    xt, yt = torch.from_numpy(np.array(x)), torch.from_numpy(np.array(y))
    res, gy = M.masking_rows_host(xt, yt, grad=True)
    assert res.audible.tolist() == [r.audible for r in r64] and res.cells.tolist() == [r.cells for r in r64]
    for i, r in enumerate(r64):
        assert abs(float(res.nmr_db[i]) - r.nmr_db) <= 1e-6 * max(1.0, abs(r.nmr_db)) and abs(float(res.over_db[i]) - r.over_db) <= 1e-6
        scale = np.abs(r.grad).max()
        assert np.abs(gy[i].numpy() - r.grad).max() <= 1e-6 * scale + 1e-30            # float32 storage of a float64 result
    got = awm_amd.masking(xt[:, None], yt[:, None])
    assert torch.equal(got.over_db, res.over_db) and torch.equal(got.audible, res.audible) and got.cells.dtype == torch.int32
    assert torch.equal(awm_amd.nmr(xt, yt), res.nmr_db) and awm_amd.nmr(xt[0], yt[0]).shape == ()
    yl = yt[:, None].clone().requires_grad_(True)
    xl = xt[:, None].clone().requires_grad_(True)
    loss = awm_amd.MaskingLoss()(xl, yl)
    assert abs(float(loss.detach()) - np.mean([r.over_db for r in r64])) <= 1e-6
    loss.backward()
    assert xl.grad is None, "the mask is not differentiated"
    want = np.stack([r.grad for r in r64]) / 3.0
    assert tuple(yl.grad.shape) == (3, 1, n) and np.abs(yl.grad[:, 0].numpy() - want).max() <= 1e-6 * np.abs(want).max()


def test_edge_rows_on_the_host():
    x, y = Y.case(1280)
    xt, yt = torch.from_numpy(np.array(x)), torch.from_numpy(np.array(y))
    short = M.masking_rows_host(xt[:, :511], yt[:, :511])
    assert torch.isnan(short.nmr_db).all() and short.over_db.tolist() == [0.0] * 3 and short.audible.tolist() == short.cells.tolist() == [0] * 3
    same, gy = M.masking_rows_host(xt, xt.clone(), grad=True)
    assert (same.nmr_db == -math.inf).all() and same.over_db.tolist() == [0.0] * 3 and same.audible.tolist() == [0] * 3
    assert same.cells.tolist() == [88] * 3 and not gy.any()
    bad = yt.clone()
    bad[1, 700] = math.nan
    res, clean = M.masking_rows_host(xt, bad), M.masking_rows_host(xt, yt)
    assert math.isnan(float(res.nmr_db[1])) and math.isnan(float(res.over_db[1])) and res.audible[1] == 0 and res.cells[1] == 0
    for i in (0, 2):
        assert res.nmr_db[i] == clean.nmr_db[i] and res.over_db[i] == clean.over_db[i] and res.audible[i] == clean.audible[i]
    for r in (Y.model(x[0][:511], y[0][:511]), Y.model(x[0], x[0]), Y.model(x[1], bad[1].numpy())):
        assert r.audible == 0
    assert Y.model(x[0], x[0]).nmr_db == -math.inf and math.isnan(Y.model(x[1], bad[1].numpy()).over_db)
    silent = M.masking_rows_host(torch.zeros(1, 1280), yt[2:3])                      # x == 0: the threshold in quiet alone
    ref = Y.model(np.zeros(1280), y[2])
    assert abs(float(silent.nmr_db[0]) - ref.nmr_db) <= 1e-5 and int(silent.audible[0]) == ref.audible


def test_refusals_on_the_host():
    import awm_amd
    x = torch.zeros(2, 2000)
    for bx, by, rate in ((x, torch.zeros(2, 1999), 16000), (x, torch.zeros(3, 2000), 16000), (x.double(), x.double(), 16000),
                         (torch.zeros(2, 2, 2000), torch.zeros(2, 2, 2000), 16000), (torch.zeros(2, 0), torch.zeros(2, 0), 16000),
                         (x, x, 0), (x, x, 16000.5), (x, x, True)):
        with pytest.raises(ValueError):
            awm_amd.masking(bx, by, rate)
    with pytest.raises(TypeError):
        awm_amd.masking(x.numpy(), x)
    for rows, n in ((0, 100), (1, 0), (1, 2 ** 34 + 1), (2 ** 20, 2 ** 30), (1.5, 10), (True, 10)):
        with pytest.raises(ValueError):
            M.masking_plan(rows, n)


# ------------------------------------------------------------------------------------------ the C boundary
def test_entry_points_are_declared_exported_and_built():
    from awm_amd import _lib
    protos = _lib.parse_header()
    assert [c for c, _ in protos["wm_masking_plan"]] == ["long long", "long long", "long long*", "long long*", "long long*", "wm_stream_t"]
    assert [a for _, a in protos["wm_masking_fwd"]] == ["x", "y", "tables", "nmr_db", "over_db", "counts", "coef", "scratch", "rows", "n", "stream"]
    assert [a for _, a in protos["wm_masking_bwd"]] == ["x", "y", "coef", "gout", "gy", "rows", "n", "stream"]
    text = open(os.path.join(PKG, "csrc", "masking.hip")).read()
    for name in ("wm_masking_plan", "wm_masking_fwd", "wm_masking_bwd"):
        assert f"int {name}(" in text
    assert "fft_dif<9>" in text and "atomic" not in text.lower().replace("no atomics", "")
    dll = _lib.lib.load()
    for name in ("wm_masking_plan", "wm_masking_fwd", "wm_masking_bwd"):
        assert hasattr(dll, name)
    import awm_amd
    for name in ("masking", "MaskingLoss", "nmr"):
        assert name in awm_amd.__all__ and hasattr(awm_amd, name)
    assert list(awm_amd.__all__[-3:]) == ["masking", "MaskingLoss", "nmr"]


def test_plan_is_a_host_query():
    for rows, n in ((1, 1), (3, 511), (3, 512), (3, 767), (3, 768), (512, 16000), (1, 57_600_000)):
        frames, chunk, need = M.masking_plan(rows, n)
        assert frames == Y.frame_count(n) and chunk >= 2 and chunk % 2 == 0
        assert need == 24 * rows * max(-(-frames // chunk), 1)
    assert M.masking_plan(1, 57_600_000)[0] == 224_999                             # an hour in one row
    assert M.masking_plan(1, 16000)[1] == M.masking_plan(512, 64000)[1], "the chunk knows nothing of the batch"


# ------------------------------------------------------------------------------------------ the wiring
def test_metric_names():
    from awm_amd import quality
    assert quality.METRICS == ("stoi", "nmr")
    assert quality.check_metrics("nmr") == ("nmr",) and quality.check_metrics(["stoi", "nmr"]) == ("stoi", "nmr")
    for bad in (("pesq",), ("nmr", "estoi"), "STOI", "NMR"):
        with pytest.raises(ValueError, match="unknown metric"):
            quality.check_metrics(bad)


def test_evaluate_robustness_key_sets():
    import awm_amd
    ident = torch.nn.Identity()
    four = ["bit_accuracy", "clean_prob", "delta_rms", "watermarked_prob"]
    new = ["audible_share", "audible_share_attack_only", "nmr_db", "nmr_db_attack_only", "nmr_rows"]
    for quality, extra in (((), []), (("stoi",), ["stoi", "stoi_attack_only", "stoi_rows"])):
        res = awm_amd.evaluate_robustness(ident, ident, [], {"a": ident}, device="cpu", quality=quality)
        assert list(res) == ["none", "a"] and all(sorted(row) == sorted(four + extra) for row in res.values())
    res = awm_amd.evaluate_robustness(ident, ident, [], {"a": ident}, device="cpu", quality=("nmr",))
    for row in res.values():
        assert sorted(row) == sorted(four + new) and row["nmr_rows"] == 0
        assert all(math.isnan(row[k]) for k in new if k != "nmr_rows")
    res = awm_amd.evaluate_robustness_by_class(ident, ident, [], {"a": ident}, device="cpu", quality=("stoi", "nmr"))
    for row in res.values():
        for per in row["by_class"].values():
            assert per["nmr_rows"] == 0 and math.isnan(per["nmr_db"]) and math.isnan(per["audible_share_attack_only"]) and per["stoi_rows"] == 0


def test_signatures():
    import awm_amd
    from awm_amd import main14b_2
    for fn in (awm_amd.forward_losses, awm_amd.train_step):
        name, par = list(inspect.signature(fn).parameters.items())[-1]
        assert name == "masking" and par.default is None
    assert "masking" not in inspect.signature(main14b_2.forward_losses).parameters
    for fn in (awm_amd.generate_watermarked_audio, awm_amd.evaluate_unseen_file):
        assert inspect.signature(fn).parameters["nmr"].default is False
    assert list(awm_amd.LOSS_WEIGHTS) == ["l1", "mel", "loud", "loc", "bce", "hf"]
