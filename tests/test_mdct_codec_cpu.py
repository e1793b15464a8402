"""Host side of the transform-codec stand-in (no GPU): the float64 yardstick itself (tests/mdct_yardstick.py), the near-tie condition the
GPU file's code comparison rests on, attacks.TransformCodec on CPU tensors, the per-row draw, argument errors of the module, of
ops.mdct_kcut and of the C ABI, the export, and the bitrate estimate.

Near ties.  The GPU test compares the kernel's int16 codes with the float64 codes exactly, except where r64 = X / step lies within
h = 8 max|r32 - r64| of a half-integer (r32 from the float32 restatement of the definition): there a float32 transform may round the
other way and the codes may differ by 1.  That exception is only honest while the excepted set is small, so its share is capped at 1 % for
EVERY input the GPU file uses -- a condition of the test, checked here, not a tolerance."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import awm_amd
from awm_amd import _lib, attacks, ops

import mdct_yardstick as Y

TIE_CAP = 0.01


# ------------------------------------------------------------------------------------------ 1. the yardstick
@pytest.mark.parametrize("M", [64, 256])
def test_yardstick_is_the_identity_without_the_quantiser(M):
    """Princen-Bradley: with kcut = M the lapped transform reconstructs every sample, the first and the last hop included"""
    rng = np.random.default_rng(1)
    for n in (1, 2, M - 1, M, M + 1, 3 * M + 7, 16000):
        x = rng.standard_normal((2, n))
        y = Y.codec(x, M, 8, M, np.zeros(2), 1.0, quantise=False)["y"]
        assert y.shape == x.shape
        assert np.abs(y - x).max() < 1e-12, (M, n, np.abs(y - x).max())


def test_yardstick_linear_map_is_symmetric():
    rng = np.random.default_rng(2)
    for M, n, kcut in ((64, 300, 64), (128, 1000, 112), (256, 1027, 224)):
        u, v = rng.standard_normal((1, n)), rng.standard_normal((1, n))
        mask = rng.integers(0, 2, (1, -(-n // M) + 1, M))
        for m in (None, mask):
            Au = Y.codec(u, M, 8, kcut, np.zeros(1), 1.0, quantise=False, mask=m)["y"]
            Av = Y.codec(v, M, 8, kcut, np.zeros(1), 1.0, quantise=False, mask=m)["y"]
            assert abs(float((Au * v).sum() - (u * Av).sum())) < 1e-11
    # codes= replaces the rounding decisions: the yardstick's own codes give its own output, others move it
    x = Y.signal(1, 600)
    a = Y.codec(x, 128, 8, 112, [20.0], 2.0 ** -15)
    b = Y.codec(x, 128, 8, 112, [20.0], 2.0 ** -15, codes=a["codes"])
    assert np.array_equal(a["y"], b["y"])
    c = Y.codec(x, 128, 8, 112, [20.0], 2.0 ** -15, codes=a["codes"] + 1)
    assert np.abs(c["y"] - a["y"]).max() > 1e-4
    assert np.abs(a["codes"]).max() <= math.sqrt(8 / 12) * 10 and (a["codes"][:, :, 112:] == 0).all()


# ------------------------------------------------------------------------------------------ 2. the near-tie condition
def test_near_tie_share_of_the_issue_cases():
    """floor_step = 2^-15, M = 256, band 8, kcut 224, SNR 10 / 20 / 30: the cases the share was first measured on (at most 7.1e-4)"""
    for rows, n in ((8, 1027), (4, 16000)):
        x = Y.signal(rows, n)
        tie, share, a, b, h = Y.near_tie(x, 256, 8, 224, Y.snr_rows(rows), 2.0 ** -15)
        differ = a["codes"] != b["codes"]
        print(f"({rows}, {n}): h {h:.3e} share {share:.3e}, float32 codes differ in {int(differ.sum())} of {differ.size}")
        assert share <= TIE_CAP
        assert not (differ & ~tie).any(), "float32 and float64 codes differ outside the excepted set"
        assert np.abs(a["codes"] - b["codes"]).max() <= 1


@pytest.mark.parametrize("rows,M,n", Y.GPU_CASES)
def test_near_tie_share_of_every_gpu_case(rows, M, n):
    """the inputs of tests/test_gpu_mdct_codec.py, with the module's default floor_step"""
    x = Y.signal(rows, n)
    tie, share, a, b, h = Y.near_tie(x, M, Y.BAND, Y.KCUT[M], Y.snr_rows(rows), Y.default_floor_step(M))
    differ = a["codes"] != b["codes"]
    print(f"rows {rows} M {M} n {n}: h {h:.3e} share {share:.3e}, float32 codes differ in {int(differ.sum())} of {differ.size}")
    assert share <= TIE_CAP
    assert not (differ & ~tie).any()
    assert Y.default_floor_step(M) == ops.mdct_default_floor_step(M)


# ------------------------------------------------------------------------------------------ 3. the module on CPU tensors
def cpu_bound(x, M, kcut, snr, floor_step, codes, ref):
    """The module's CPU path is a float32 evaluation of the definition, as the yardstick's dtype=float32 mode is: with the SAME codes the two
    differ from float64 by the roundings of their float32 sums alone.  E32 = the largest error of the yardstick's float32 mode against
    float64 on this input and these codes; 4 E32 covers another summation order (the factor the GPU file uses), plus one float32 ulp of the
    largest output."""
    b = Y.codec(x, M, 8, kcut, snr, floor_step, codes=codes, dtype=np.float32)
    e = float(np.abs(b["y"].astype(np.float64) - ref["y"]).max())
    return 4 * e + float(np.spacing(np.float32(np.abs(ref["y"]).max())))


@pytest.mark.parametrize("shape,hop", [((3, 1, 1027), 256), ((2, 700), 128), ((515,), 128), ((1, 1, 2051), 512)])
def test_cpu_path_against_the_yardstick(shape, hop):
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    x = Y.signal(rows, shape[-1])
    att = awm_amd.TransformCodec(snr_db=(10, 30), bandwidth_hz=7000, hop=hop, seed=4)
    assert att.kcut == Y.KCUT[hop] and att.floor_step == Y.default_floor_step(hop)
    y, codes = att._host(torch.from_numpy(x).reshape(shape), torch.from_numpy(attacks.row_snr_db(4, 0, np.arange(rows), (10, 30))))
    out = att(torch.from_numpy(x).reshape(shape))
    assert out.shape == shape and out.dtype == torch.float32 and torch.equal(out, y)
    snr = att.last_snr_db.numpy()
    assert snr.shape == (rows,) and snr.dtype == np.float32
    tie, share, a, b, h = Y.near_tie(x, hop, 8, att.kcut, snr, att.floor_step)
    got = codes.numpy().astype(np.int64)
    assert got.shape == a["codes"].shape
    assert share <= TIE_CAP and np.array_equal(got[~tie], a["codes"][~tie]) and np.abs(got - a["codes"]).max() <= 1
    ref = Y.codec(x, hop, 8, att.kcut, snr, att.floor_step, codes=got)
    err = np.abs(out.numpy().reshape(rows, -1).astype(np.float64) - ref["y"]).max()
    bound = cpu_bound(x, hop, att.kcut, snr, att.floor_step, got, ref)
    print(f"{shape} hop {hop}: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.abs(out.numpy().reshape(rows, -1) - x).max() > 1e-3, "the quantiser did something"


def test_fine_quantiser_is_near_the_identity_and_the_cut_removes_the_top():
    x = Y.signal(2, 4000)
    y = awm_amd.TransformCodec(snr_db=60)(torch.from_numpy(x)).numpy()
    assert np.abs(y - x).max() < 2e-3 and np.sqrt(((y - x) ** 2).mean()) < 3e-4
    t = np.arange(4000)
    tone = (0.3 * np.sin(2 * np.pi * 6000 * t / 16000)).astype(np.float32)[None]
    cut = awm_amd.TransformCodec(snr_db=60, bandwidth_hz=4000)(torch.from_numpy(tone)).numpy()
    assert np.sqrt((cut[:, 512:-512] ** 2).mean()) < 0.01 * np.sqrt((tone ** 2).mean()), "a 6 kHz tone does not pass a 4 kHz cut"


# ------------------------------------------------------------------------------------------ 4. the draw
def test_per_row_draw_is_the_fourth_philox_word():
    seed, draw, rows = (5 << 32) + 9, 3, np.arange(7, 13)
    got = attacks.row_snr_db(seed, draw, rows, (10, 30))
    assert got.dtype == np.float32
    for r, v in zip(rows, got):
        o = attacks.philox4x32_10((0xFFFFFFFF, 0xFFFFFFFF, int(r), draw), (9, 5))
        u = ((int(o[3]) >> 9) + 0.5) * 2.0 ** -23
        assert v == np.float32(20.0 * u + 10.0)
    assert ((got >= 10) & (got <= 30)).all() and got.std() > 1
    # Distortion's three words are the other three: the same counter, no shared number
    g, s, _ = attacks.row_parameters(seed, draw, rows, (10.0, 30.0, 10.0, 30.0, 1.0))
    assert not np.any(g == got) and not np.any(s == got)
    assert np.array_equal(attacks.row_snr_db(seed, draw, rows, (25, 25)), np.full(6, 25, dtype=np.float32)), "a number fixes the quality"


def test_row0_cuts_reset_and_last_snr_db():
    x = torch.from_numpy(Y.signal(5, 700))
    att = awm_amd.TransformCodec(seed=11, hop=128)
    assert att.draw == 0
    a, snr_a = att(x), att.last_snr_db.clone()
    b = att(x)
    assert att.draw == 2 and not torch.equal(a, b), "every call draws fresh qualities"
    assert torch.equal(att.reset()(x), a) and torch.equal(att.reset(1)(x), b)
    pieces = [att.reset()(x[0:2]), att.reset()(x[2:3], row0=2), att.reset()(x[3:], row0=3)]
    assert torch.equal(torch.cat(pieces), a), "a batch cut into pieces, numbered by row0, is the whole batch"
    assert torch.equal(att.last_snr_db, snr_a[3:])
    assert not torch.equal(att.reset()(x[3:]), a[3:])
    assert torch.equal(awm_amd.TransformCodec(seed=11, hop=128)(x), a) and not torch.equal(awm_amd.TransformCodec(seed=12, hop=128)(x), a)
    fixed = awm_amd.TransformCodec(snr_db=20, hop=128)
    assert torch.equal(fixed(x), fixed(x)) and torch.equal(fixed.last_snr_db, torch.full((5,), 20.0))
    # inside Sequential, after another module
    chain = torch.nn.Sequential(awm_amd.Distortion(gain_db=0, snr_db=None), awm_amd.TransformCodec(snr_db=20, hop=128))
    assert torch.equal(chain(x), fixed(x))


# ------------------------------------------------------------------------------------------ 5. arguments
def test_module_argument_errors():
    T = awm_amd.TransformCodec
    for kw in (dict(snr_db=(30, 10)), dict(snr_db=(-1, 10)), dict(snr_db=61), dict(snr_db=(1, 2, 3)), dict(snr_db=float("nan")),
               dict(snr_db="high"), dict(snr_db=True), dict(hop=64), dict(hop=300), dict(hop=1024), dict(band=3), dict(band=64),
               dict(bandwidth_hz=0), dict(bandwidth_hz=-5), dict(bandwidth_hz=8001), dict(bandwidth_hz=float("inf")),
               dict(bandwidth_hz=100), dict(bandwidth_hz="wide"), dict(sample_rate=0, bandwidth_hz=4000), dict(seed=1.5),
               dict(grad="reference"), dict(grad=None)):
        with pytest.raises(ValueError):
            T(**kw)
    att = T()
    for bad in (torch.zeros(2, 2, 2, 2), torch.zeros(0), torch.zeros(2, 0)):
        with pytest.raises(ValueError):
            att(bad)
    with pytest.raises(TypeError):
        att([0.0, 1.0])
    assert att.draw == 0, "a refused call draws nothing"
    for bad in (-1, 2 ** 32, 1.0):
        with pytest.raises(ValueError):
            att(torch.zeros(2, 8), row0=bad)
        with pytest.raises(ValueError):
            att.reset(bad)
    assert "grad='straight_through'" in repr(att) and "hop=256" in repr(att)
    assert awm_amd.attacks.TransformCodec is T and "TransformCodec" in awm_amd.__all__
    assert "stand-in" in T.__doc__.lower() and "unmeasured" in T.__doc__.lower()


def test_kcut_from_the_bandwidth():
    assert ops.mdct_kcut(256, 8) == 256 and ops.mdct_kcut(512, 32, None) == 512
    assert ops.mdct_kcut(256, 8, 7000) == 224                                    # floor(7000 * 512 / 16000) = 224
    assert ops.mdct_kcut(256, 8, 7100) == 224                                    # 227 -> down to the band
    assert ops.mdct_kcut(256, 32, 7100) == 224 and ops.mdct_kcut(256, 32, 6999) == 192
    assert ops.mdct_kcut(128, 4, 8000) == 128 and ops.mdct_kcut(512, 16, 11025, 44100) == 256
    assert ops.mdct_kcut(256, 8, 250) == 8
    with pytest.raises(ValueError):
        ops.mdct_kcut(256, 8, 249)                                               # less than one band
    assert ops.mdct_frames(1, 256) == 2 and ops.mdct_frames(256, 256) == 2 and ops.mdct_frames(257, 256) == 3
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.mdct_codec(torch.zeros(2, 100), torch.zeros(2))


def test_launcher_rejects_bad_arguments_without_a_gpu():
    """hipErrorInvalidValue (1) comes back before anything is launched, so these calls need no device"""
    x, y, c, m, s = 1 << 20, 1 << 22, 1 << 24, 1 << 26, 1 << 28                  # made-up, never dereferenced addresses
    fs = 2.0 ** -15
    nan, inf = float("nan"), float("inf")
    for args in ((x, y, c, None, s, 0, 1000, 256, 8, 256, fs, 1, None),            # rows < 1
                 (x, y, c, None, s, 2, 0, 256, 8, 256, fs, 1, None),               # n < 1
                 (x, y, c, None, s, 1, (1 << 34) + 1, 256, 8, 256, fs, 1, None),   # n above 2^34
                 (x, y, c, None, s, 2, 1000, 64, 8, 64, fs, 1, None),              # M outside its set
                 (x, y, c, None, s, 2, 1000, 384, 8, 256, fs, 1, None),
                 (x, y, c, None, s, 2, 1000, 1024, 8, 256, fs, 1, None),
                 (x, y, c, None, s, 2, 1000, 256, 2, 256, fs, 1, None),            # band outside its set
                 (x, y, c, None, s, 2, 1000, 256, 12, 252, fs, 1, None),
                 (x, y, c, None, s, 2, 1000, 256, 64, 256, fs, 1, None),
                 (x, y, c, None, s, 2, 1000, 256, 8, 0, fs, 1, None),              # kcut below one band
                 (x, y, c, None, s, 2, 1000, 256, 8, 264, fs, 1, None),            # above M
                 (x, y, c, None, s, 2, 1000, 256, 8, 100, fs, 1, None),            # not a multiple of band
                 (x, y, c, None, s, 2, 1000, 256, 8, 256, 0.0, 1, None),           # floor_step
                 (x, y, c, None, s, 2, 1000, 256, 8, 256, -fs, 1, None),
                 (x, y, c, None, s, 2, 1000, 256, 8, 256, nan, 1, None),
                 (x, y, c, None, s, 2, 1000, 256, 8, 256, inf, 1, None),
                 (None, y, c, None, s, 2, 1000, 256, 8, 256, fs, 1, None),         # null pointers
                 (x, None, c, None, s, 2, 1000, 256, 8, 256, fs, 1, None),
                 (x, y, c, None, None, 2, 1000, 256, 8, 256, fs, 1, None),
                 (x + 2, y, c, None, s, 2, 1000, 256, 8, 256, fs, 1, None),        # misaligned
                 (x, y + 1, c, None, s, 2, 1000, 256, 8, 256, fs, 1, None),
                 (x, y, c + 1, None, s, 2, 1000, 256, 8, 256, fs, 1, None),
                 (x, y, None, m + 1, s, 2, 1000, 256, 8, 256, fs, 0, None),
                 (x, y, c, None, s + 2, 2, 1000, 256, 8, 256, fs, 1, None),
                 (x, x, c, None, s, 2, 1000, 256, 8, 256, fs, 1, None),            # in place
                 (x, x + 7996, c, None, s, 2, 1000, 256, 8, 256, fs, 1, None),     # y overlaps the last float of x
                 (x, y, y + 4000, None, s, 2, 1000, 256, 8, 256, fs, 1, None),     # the codes inside y
                 (x, y, None, y, s, 2, 1000, 256, 8, 256, fs, 0, None),            # the mask is y
                 (x, y, c, None, s, 2, 1000, 256, 8, 256, fs, 0, None)):           # codes without the quantiser
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm_amd.lib.wm_mdct_codec(*args)


def test_plan_is_a_function_of_the_shape():
    """64 frames per workgroup where that pads no more than 32 do; hop 512 stays at 32"""
    for n, hop, want in ((1, 256, (32, 1)), (16000, 256, (64, 1)), (16000, 128, (64, 2)), (16000, 512, (32, 2)), (1027, 256, (32, 1)),
                         (31 * 256, 256, (32, 1)), (31 * 256 + 1, 256, (64, 1)), (63 * 256 + 1, 256, (32, 3)), (24059, 256, (64, 2)),
                         (10 ** 7, 512, (32, 631))):
        assert ops.mdct_plan(n, hop) == want, (n, hop, ops.mdct_plan(n, hop))
    import ctypes
    a, b = ctypes.c_int(0), ctypes.c_longlong(0)
    for n, hop in ((0, 256), (100, 64), ((1 << 34) + 1, 256)):
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm_amd.lib.wm_mdct_codec_plan(n, hop, ctypes.addressof(a), ctypes.addressof(b), None)
    with pytest.raises(RuntimeError, match="hipError 1$"):
        awm_amd.lib.wm_mdct_codec_plan(100, 256, None, ctypes.addressof(b), None)


def test_entry_point_is_declared_and_exported():
    protos = _lib.parse_header()
    assert "wm_mdct_codec" in protos
    assert [name for _, name in protos["wm_mdct_codec"]] == ["x", "y", "codes_out", "mask_in", "snr_db", "rows", "n", "M", "band", "kcut",
                                                            "floor_step", "quantise", "stream"]
    assert os.path.exists(_lib.LIB_PATH), "build with __graft_entry__.build()"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "wm_mdct_codec"), "wm_mdct_codec declared in include/wm_hip.h but not exported"
    assert hasattr(ops, "mdct_codec") and hasattr(ops, "MdctCodecFn")
    assert "not differentiated" in " ".join(ops.MdctCodecFn.__doc__.lower().split())


# ------------------------------------------------------------------------------------------ 6. the bitrate estimate
def test_estimate_kbps_on_hand_made_codes():
    hop, band, kcut, sr = 128, 4, 8, 16000
    codes = torch.zeros(2, 3, hop, dtype=torch.int16)
    # band 0: the 24 pooled values are 12 zeros, 6 ones, 6 minus-ones -> H = 1.5 bits; band 1: all 7 -> H = 0; above kcut: ignored
    codes[:, :, :4] = torch.tensor([0, 0, 1, -1], dtype=torch.int16)
    codes[:, :, 4:8] = 7
    codes[:, :, 8:] = 123
    want = ((4 * 1.5 + 8) + (4 * 0.0 + 8)) * sr / hop / 1000.0
    assert attacks.code_entropy_kbps(codes, band, kcut, hop, sr) == pytest.approx(want, rel=1e-12)
    # against numpy on random codes
    rng = np.random.default_rng(3)
    c = rng.integers(-5, 6, (3, 9, 256)).astype(np.int16)
    bits = 0.0
    for b in range(224 // 8):
        _, cnt = np.unique(c[:, :, 8 * b:8 * b + 8], return_counts=True)
        p = cnt / cnt.sum()
        bits += 8 * float(-(p * np.log2(p)).sum()) + 8
    assert attacks.code_entropy_kbps(torch.from_numpy(c), 8, 224, 256, 16000) == pytest.approx(bits * 16000 / 256 / 1000, rel=1e-12)
    with pytest.raises(ValueError):
        attacks.code_entropy_kbps(torch.zeros(2, 128, dtype=torch.int16), 4, 8, 128, 16000)
    # the module: a coarser quantiser costs fewer bits; the draw is left where it was
    x = torch.from_numpy(Y.signal(2, 4000))
    lo, hi = awm_amd.TransformCodec(snr_db=10), awm_amd.TransformCodec(snr_db=40)
    k_lo, k_hi = lo.estimate_kbps(x), hi.estimate_kbps(x)
    print(f"estimate: {k_lo:.1f} kbit/s at 10 dB, {k_hi:.1f} kbit/s at 40 dB")
    assert 0 < k_lo < k_hi and lo.draw == 0
    assert "estimate" in awm_amd.TransformCodec.estimate_kbps.__doc__.lower()
