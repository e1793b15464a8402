"""The predictive speech-codec stand-in without a GPU: the facts about the yardstick of tests/lpc_yardstick.py that
tests/test_gpu_lpc_codec.py leans on (near-tie shares, the coefficient bound in four float32 summation orders, the adjoint identity,
Levinson-Durbin against a dense solve), the draw (word o3 of the "param2" counter), the CPU path of attacks.LpcCodec against the
yardstick's float32 mode, argument validation, and the C boundary (the launcher refuses bad arguments before any launch, so those calls
need no device)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import awm_amd
from awm_amd import _lib, attacks, ops

import draw_yardstick as D
import lpc_yardstick as Y

CPU_CASES = [(3, 160, 2, 4 * 160 + 3), (3, 160, 10, 4 * 160 + 3), (3, 320, 16, 4 * 320 + 3), (3, 640, 16, 3 * 640 + 5), (3, 320, 16, 16000)]
SIGNALS = {"plain": Y.signal_plain, "speech": Y.signal_speech}


# ------------------------------------------------------------------------------------------ the yardstick's own facts
@pytest.mark.parametrize("name", list(SIGNALS))
@pytest.mark.parametrize("rows,L,p,n", CPU_CASES)
def test_near_tie_share_is_small(name, rows, L, p, n):
    x = SIGNALS[name](rows, n)
    c32 = Y.analyse(x, L, p, np.float32)["coeffs"]
    tie, share, codes, h = Y.near_tie(x, c32, L, Y.snr_rows(rows))
    print(f"{name} L {L} p {p} n {n}: near-tie share {share:.2e}, h {h:.2e}, zero codes {(codes == 0).mean():.2f}, max |q| {np.abs(codes).max()}")
    assert share <= 0.01 and np.abs(codes).max() <= np.sqrt(L / 12.0) * 1e3 < 32767


def test_near_tie_share_of_the_degenerate_rows():
    n, L, p = 4 * 320 + 3, 320, 16
    x = Y.degenerate(n)
    c32 = Y.analyse(x, L, p, np.float32)["coeffs"]
    assert np.isfinite(c32).all() and not c32[0].any()
    tie, share, codes, h = Y.near_tie(x, c32, L, Y.snr_rows(4))
    print(f"degenerate rows: near-tie share {share:.2e}, h {h:.2e}")
    assert share <= 0.01 and not codes[:2].any()


@pytest.mark.parametrize("rows,L,p,n", CPU_CASES)
def test_float32_coefficients_stay_inside_the_bound_in_four_orders(rows, L, p, n):
    """signal_plain: every float32 summation order of the autocorrelation stays within the first-order bound (and uses little of it)"""
    x = Y.signal_plain(rows, n)
    c64, bound = Y.coeff_bound(x, L, p)
    assert (bound > 0).all() and bound.max() < 0.02, "the bound says something on this input"
    for order in Y.ORDERS:
        c32 = Y.analyse(x, L, p, np.float32, order)["coeffs"]
        ratio = (np.abs(c32 - c64) / bound).max()
        print(f"L {L} p {p} n {n} {order}: max err / bound {ratio:.4f}, bound {bound.min():.1e} .. {bound.max():.1e}")
        assert ratio <= 1.0


@pytest.mark.parametrize("rows,L,p,n", CPU_CASES)
def test_float32_prediction_gain_in_four_orders(rows, L, p, n):
    """signal_speech: the systems are too ill-conditioned for the bound, but the prediction gain is second order in the coefficients"""
    x = Y.signal_speech(rows, n)
    g64 = Y.prediction_gain_db(x, Y.analyse(x, L, p)["coeffs"], L)
    assert (g64 > (8 if p == 2 else 20)).all(), g64
    for order in Y.ORDERS:
        g32 = Y.prediction_gain_db(x, Y.analyse(x, L, p, np.float32, order)["coeffs"], L)
        print(f"L {L} p {p} n {n} {order}: gain {g64.round(2)}, float32 off by {np.abs(g32 - g64).max():.2e} dB")
        assert np.abs(g32 - g64).max() <= 0.05


@pytest.mark.parametrize("L,p,n", [(160, 10, 4 * 160 + 3), (320, 16, 4 * 320 + 3)])
def test_adjoint_identity_in_float64(L, p, n):
    x = Y.signal_speech(3, n)
    c = Y.analyse(x, L, p, np.float32)["coeffs"]
    codes = Y.codec(x, c, L, Y.snr_rows(3), synth=False)["codes"]
    rng = np.random.default_rng(L)
    u, g = rng.standard_normal((3, n)), rng.standard_normal((3, n))
    for mask in (None, codes != 0):
        Au = Y.codec(u, c, L, None, quantise=False, mask=mask)["y"]
        lhs, rhs = float((Au * g).sum()), float((u * Y.adjoint(g, c, L, mask)).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), float(np.abs(Au * g).sum()) * 1e-3)
    assert np.abs(Y.adjoint(g, c, L) - g).max() <= 1e-9 * np.abs(g).max(), "without a mask the map is the identity"
    # dense check on a short row: the matrix of the forward map, column by column
    m = L + 40
    cm, mk = c[:1, :2], (codes[:1, :m] != 0)
    A = np.stack([Y.codec(np.eye(m)[i:i + 1], cm, L, None, quantise=False, mask=mk)["y"][0] for i in range(m)], axis=1)
    gm = g[:1, :m]
    assert np.abs(A.T @ gm[0] - Y.adjoint(gm, cm, L, mk)[0]).max() <= 1e-12 * np.abs(A).max() * np.abs(gm).sum()


def test_levinson_against_a_dense_solve():
    x = Y.signal_plain(2, 4 * 320 + 3)
    for L, p in ((160, 2), (160, 10), (320, 16)):
        ref = Y.analyse(x, L, p)
        expand = Y.tables(p)[1].astype(np.float64)
        idx = np.abs(np.arange(p)[:, None] - np.arange(p)[None, :])
        for r in range(2):
            for f in range(ref["Rc"].shape[1]):
                Rc = ref["Rc"][r, f]
                want = np.linalg.solve(Rc[idx], -Rc[1:]) * expand
                assert np.abs(ref["coeffs"][r, f] - want).max() <= 1e-9
    # an all-zero frame and a frame whose recursion must stop
    assert not Y.levinson(np.zeros((1, 5)), 4, np.float64).any()
    a = Y.levinson(np.array([[1.0, 0.5, 2.0, 0.1, 0.1]]), 4, np.float64)
    assert a[0, 0] == -0.5 and not a[0, 1:].any(), "the step with |k| >= 1 and everything after it stay 0"


def test_tables_and_frames():
    for p, sr in ((2, 16000), (10, 8000), (16, 16000)):
        lag, expand = ops.lpc_tables(p, sr)
        assert lag.dtype == torch.float32 and tuple(lag.shape) == (p + 1,) and tuple(expand.shape) == (p,) and ops.lpc_tables(p, sr)[0] is lag
        wl, we = Y.tables(p, sr)
        assert np.array_equal(lag.numpy(), wl) and np.array_equal(expand.numpy(), we)
        assert lag[0] == np.float32(1.0001) and (np.diff(lag.numpy()) < 0).all() and expand[0] == np.float32(0.994)
    for n, L in ((1, 160), (159, 160), (160, 160), (161, 160), (16000, 320), (1925, 640)):
        assert ops.lpc_frames(n, L) == Y.frames(n, L)
    assert ops.lpc_frames(161, 160) == 2 and ops.LPC_GRAD_MODES == ("straight_through", "dead_zone")


# ------------------------------------------------------------------------------------------ draws and counters
def test_the_draw_is_word_o3_of_the_param2_counter():
    seed, draw, rows = (5 << 32) + 9, 3, np.arange(7, 40)
    s = attacks.row_lpc_snr_db(seed, draw, rows, (10, 30))
    o = D.philox4x32_10((*D.PARAM2, rows, draw), D.key_of(seed))
    assert s.dtype == np.float32 and np.array_equal(s, D.affine32((10, 30), D.unit(o[3])))
    assert (s >= 10).all() and (s <= 30).all() and len(set(s)) == 33
    # the other three words stay Reverb's and Convolved's
    rt60, drr = attacks.row_reverb_params(seed, draw, rows, (0.2, 0.8), (0.0, 10.0))
    assert np.array_equal(rt60, D.affine32((0.2, 0.8), D.unit(o[0]))) and np.array_equal(drr, D.affine32((0.0, 10.0), D.unit(o[1])))
    assert np.array_equal(attacks.row_bank_index(seed, draw, rows, 5), np.floor(D.unit(o[2]) * 5).astype(np.int64))
    assert not np.array_equal(o[3], o[2]) and not np.array_equal(s, attacks.row_snr_db(seed, draw, rows, (10, 30)))
    assert attacks.FAMILIES["param2"] == D.PARAM2 and {k: v for k, v in attacks.FAMILIES.items() if v[0] is not None} == D.FAMILIES


# ------------------------------------------------------------------------------------------ the module's CPU path
@pytest.mark.parametrize("name", list(SIGNALS))
@pytest.mark.parametrize("L,p,n", [(160, 10, 4 * 160 + 3), (320, 16, 4 * 320 + 3), (640, 16, 3 * 640 + 5)])
def test_cpu_path_against_the_yardstick(name, L, p, n):
    """coefficients: the float32 mode's own within the rule of the GPU test (bound, or prediction gain); codes and output: the float32
    mode teacher-forced with the module's coefficients"""
    x = np.array(SIGNALS[name](3, n))
    snr = Y.snr_rows(3)
    y, a, q = attacks._lpc_rows_host(x, snr, L, p, 16000, Y.FLOOR_STEP)
    assert y.dtype == np.float32 and y.shape == x.shape and a.shape == (3, Y.frames(n, L), p) and q.dtype == np.int16
    if name == "plain":
        c64, bound = Y.coeff_bound(x, L, p)
        assert (np.abs(a - c64) <= bound).all()
    else:
        assert np.abs(Y.prediction_gain_db(x, a, L) - Y.prediction_gain_db(x, Y.analyse(x, L, p)["coeffs"], L)).max() <= 0.05
    tie, share, codes64, h = Y.near_tie(x, a, L, snr)
    differ = q.astype(np.int64) != codes64
    assert not (differ & ~tie).any() and np.abs(q.astype(np.int64) - codes64).max() <= 1
    e, y64 = Y.e32_output(x, a, L, snr, q)
    assert np.abs(y - y64).max() <= 4 * e + np.spacing(np.float32(np.abs(x).max()))


def test_module_draws_rewinds_and_numbers_rows():
    x = torch.from_numpy(np.array(Y.signal_speech(4, 700))).view(4, 1, 700)
    att = awm_amd.LpcCodec(snr_db=(10, 30), frame=160, order=10, seed=5)
    y = att(x)
    assert y.shape == x.shape and y.dtype == torch.float32 and att.draw == 1
    assert np.array_equal(att.last_snr_db.numpy(), attacks.row_lpc_snr_db(5, 0, np.arange(4), (10, 30)))
    assert torch.equal(att.reset()(x), y) and not torch.equal(att(x), y), "reset rewinds; the next draw differs"
    pieces = torch.cat([att.reset()(x[:1]), att.reset()(x[1:], row0=1)])
    assert torch.equal(pieces, y), "a batch cut into pieces, numbered by row0, is the whole batch"
    snr = 10 * torch.log10(x.pow(2).sum(-1) / (y - x).pow(2).sum(-1)).view(-1)
    assert bool(((snr - att.reset()(x).new_tensor(attacks.row_lpc_snr_db(5, 0, np.arange(4), (10, 30)))).abs() < 8).all()), snr
    fixed = awm_amd.LpcCodec(snr_db=20)
    fixed(x)
    assert (fixed.last_snr_db == 20).all() and "snr_db=(20.0, 20.0)" in repr(fixed) and "frame=320" in repr(fixed)
    assert (x - awm_amd.LpcCodec(snr_db=60)(x)).abs().max() < 1e-3 and awm_amd.LpcCodec(20)(x.view(4, 700)).shape == (4, 700)


def test_inside_sequential_with_the_pcm_codec():
    x = torch.from_numpy(np.array(Y.signal_speech(2, 600))).reshape(2, 1, 600)
    chain = torch.nn.Sequential(awm_amd.Distortion(seed=3), awm_amd.LpcCodec(20, frame=160), awm_amd.PcmCodec())
    y = chain(x)
    assert y.shape == x.shape and bool(torch.isfinite(y).all()) and chain[1].draw == 1


# ------------------------------------------------------------------------------------------ refusals, the interface and the build
def test_constructor_and_forward_refusals():
    for v in (-1, 61, (5, 61), (30, 10), True, "high", float("nan"), (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError):
            awm_amd.LpcCodec(snr_db=v)
    for kw in (dict(frame=256), dict(frame=320.0), dict(frame=True), dict(order=1), dict(order=17), dict(order=8.0), dict(order=True),
               dict(sample_rate=0), dict(sample_rate=float("inf")), dict(seed=1.5), dict(grad="through")):
        with pytest.raises(ValueError):
            awm_amd.LpcCodec(**kw)
    att = awm_amd.LpcCodec()
    for bad in (-1, 2 ** 32 - 1, 0.0, True):
        with pytest.raises(ValueError):
            att(torch.zeros(2, 100), row0=bad)
    with pytest.raises(ValueError):
        att(torch.zeros(2, 1, 1, 100))
    with pytest.raises(TypeError):
        att([0.0] * 100)
    assert att.draw == 0, "a call that raises consumes no draw"


def test_ops_refuse_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lpc_codec(torch.zeros(2, 100), torch.ones(2))


def test_launcher_rejects_bad_arguments_without_a_gpu():
    """hipErrorInvalidValue (1) comes back before anything is launched, so these calls need no device"""
    for args in Y.BAD_ARGS:
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm_amd.lib.wm_lpc_codec(*args)


def test_entry_point_is_declared_exported_and_built():
    protos = _lib.parse_header()
    assert [name for _, name in protos["wm_lpc_codec"]] == ["x", "y", "coeffs_in", "coeffs_out", "codes_out", "mask_in", "snr_db", "lag",
                                                            "expand", "rows", "n", "L", "p", "floor_step", "quantise", "adjoint", "stream"]
    assert [c for c, _ in protos["wm_lpc_codec"]][:6] == ["const float*", "float*", "const float*", "float*", "void*", "const void*"]
    assert os.path.exists(_lib.LIB_PATH), "build with __graft_entry__.build()"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "wm_lpc_codec"), "wm_lpc_codec declared in include/wm_hip.h but not exported"
    assert "LpcCodec" in awm_amd.__all__ and awm_amd.LpcCodec is attacks.LpcCodec
    build = open(os.path.join(_lib._PKG_DIR, "csrc", "build.sh")).read()
    assert "lpc_codec" in build.split("for f in")[1].split(";")[0].split()
    assert os.path.exists(os.path.join(_lib._PKG_DIR, "csrc", "lpc_codec.hip"))
