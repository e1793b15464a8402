"""The reverb / echo attack without a GPU: the host restatements (attacks.rir_taps, row_reverb_params, row_bank_index) against the float64
yardstick of tests/fir_yardstick.py, the Philox counter domains, the CPU paths of attacks.Convolved / Reverb, echo_ir, argument
validation, and the C boundary (the launchers refuse bad arguments before any launch, so those calls need no device)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import awm_amd
from awm_amd import _lib, attacks, ops

import fir_yardstick as Y

RIR_CASES = [(K, rt60, drr) for K in (1, 2, 33, 2048, 8192) for rt60, drr in ((0.05, 0.0), (0.3, 10.0), (0.6, 20.0))]


# ------------------------------------------------------------------------------------------ the yardstick itself
def test_adjoint_is_flip_h_flip_in_float64():
    """<H u, v> = <u, H^T v> with H^T written as flip . H . flip, below 1e-11"""
    rng = np.random.default_rng(3)
    for n, K in ((1, 1), (40, 100), (1000, 257), (4099, 64)):
        u, v, h = rng.standard_normal((2, n)), rng.standard_normal((2, n)), rng.standard_normal((2, K))
        lhs, rhs = (Y.fir(u, h) * v).sum(), (u * Y.fir_adjoint(v, h)).sum()
        assert abs(lhs - rhs) <= 1e-11 * max(1.0, abs(lhs)), (n, K, lhs, rhs)
        dense = np.array([[h[0][t - s] if 0 <= t - s < K else 0.0 for s in range(min(n, 50))] for t in range(min(n, 50))])
        np.testing.assert_allclose(Y.fir_adjoint(v[:1, :50], h[0])[0], dense.T @ v[0, :50], atol=1e-11)


def test_integer_convolution_is_exact_in_float32():
    """the GPU test's claim: float32 np.convolve reproduces the int64 result on these inputs"""
    x, h = Y.int_case(3, 4099, 1000)
    assert np.array_equal(Y.fir(x.astype(np.float32), h.astype(np.float32)), Y.fir(x, h))
    assert np.abs(Y.fir(np.abs(x), np.abs(h))).max() < 2 ** 24


# ------------------------------------------------------------------------------------------ host restatements
@pytest.mark.parametrize("K,rt60,drr", RIR_CASES)
def test_rir_taps_against_the_yardstick(K, rt60, drr):
    seed, draw, row = (7 << 32) + 5, 3, 11
    h = attacks.rir_taps(seed, draw, row, rt60, drr, K, 16000)
    ref, env = Y.rir(seed, draw, row, rt60, drr, K, 16000.0)
    assert h.dtype == np.float64 and h.shape == (K,)
    assert np.abs(h - ref).max() <= 1e-14
    w = 10.0 ** (-float(np.float32(drr)) / 10.0)
    if K > 1:
        assert abs((h * h).sum() - 1.0) <= 1e-12 and abs((h[1:] ** 2).sum() / h[0] ** 2 - w) <= 1e-12 * w
        c = 3.0 * np.log(10.0) / (float(np.float32(rt60)) * 16000.0)
        assert abs(np.log(env[1] / env[-1]) - (K - 2) * c) <= 1e-9 * max(1.0, (K - 2) * c), "60 dB in rt60"
    else:
        assert h[0] == 1.0


def test_rir_degenerate_rows():
    for kw in (dict(rt60=0.0), dict(rt60=-1.0), dict(drr_db=float("nan")), dict(drr_db=float("inf")), dict(rt60=1e-7)):
        a = dict(rt60=0.3, drr_db=6.0)
        a.update(kw)
        h = attacks.rir_taps(1, 0, 0, a["rt60"], a["drr_db"], 64, 16000)
        assert h[0] == 1.0 and not h[1:].any(), kw


def test_row_parameters_against_the_yardstick():
    seed, draw, rows = (5 << 32) + 9, 3, np.arange(7, 40)
    rt60, drr = attacks.row_reverb_params(seed, draw, rows, (0.1, 0.4), (0, 12))
    r64, d64 = Y.reverb_params(seed, draw, rows, (0.1, 0.4), (0, 12))
    assert rt60.dtype == drr.dtype == np.float32
    assert np.array_equal(rt60, r64) and np.array_equal(drr, d64)
    assert (rt60 >= np.float32(0.1)).all() and (rt60 <= np.float32(0.4)).all() and rt60.std() > 0.05
    fixed = attacks.row_reverb_params(seed, draw, rows, (0.25, 0.25), (6, 6))
    assert (fixed[0] == np.float32(0.25)).all() and (fixed[1] == np.float32(6)).all()
    idx = attacks.row_bank_index(seed, draw, rows, 5)
    assert np.array_equal(idx, Y.bank_index(seed, draw, rows, 5)) and idx.min() >= 0 and idx.max() <= 4 and len(set(idx)) == 5


def test_counter_domains_never_coincide():
    """for one (seed, draw, row): Distortion's samples (q, 0), its parameters (~0, ~0), Reverb's parameters (~0 - 1, ~0), the taps of a
    response (k >> 2, ~0 - 1) -- the first two words differ pairwise, for every q a row of 2^34 samples and every k a response can have"""
    q_max, k_max = (1 << 34) - 1 >> 2, ops.FIR_MAX_TAPS - 1 >> 2
    assert q_max < 1 << 32, "a sample counter's high word is 0"
    samples = lambda q: (q & 0xFFFFFFFF, q >> 32)
    taps = lambda k4: (k4, Y.RIR_HIGH)
    assert samples(q_max)[1] == Y.SAMPLE_HIGH == 0 and Y.RIR_HIGH != 0
    assert Y.PARAM != Y.PARAM2 and Y.PARAM[1] != Y.RIR_HIGH and Y.PARAM2[1] != Y.RIR_HIGH and Y.PARAM[1] != 0 and Y.PARAM2[1] != 0
    assert attacks.FAMILIES["param"] == Y.PARAM
    assert attacks.FAMILIES["param2"] == Y.PARAM2 and attacks.FAMILIES["rir_tap"] == (None, Y.RIR_HIGH)
    assert taps(k_max)[0] < Y.PARAM2[0], "a tap counter's first word stays far below the parameter counters'"
    # and the numbers differ: the same (seed, draw, row) through the four domains
    key = Y.key_of(12345)
    words = [tuple(Y.philox4x32_10((c0, c1, 9, 2), key).tolist()) for c0, c1 in (samples(0), taps(0), Y.PARAM, Y.PARAM2)]
    assert len(set(words)) == 4
    # the package's normals with the tap counter are the yardstick's
    assert np.array_equal(attacks._normals(12345, 2, 9, 37, "rir_tap"), Y.normals(12345, 2, 9, 37, Y.RIR_HIGH))
    assert np.array_equal(attacks.normal_noise(12345, 2, 9, 37), Y.normals(12345, 2, 9, 37, 0))


# ------------------------------------------------------------------------------------------ CPU module paths
@pytest.mark.parametrize("shape", [(3, 1, 700), (2, 450), (300,)])
def test_convolved_cpu_path_against_float64(shape):
    rng = np.random.default_rng(4)
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    x = rng.standard_normal(shape).astype(np.float32)
    h = Y.rir(1, 0, 0, 0.3, 6.0, 129, 16000.0)[0].astype(np.float32)
    y = awm_amd.Convolved(torch.from_numpy(h))(torch.from_numpy(x))
    assert y.shape == x.shape and y.dtype == torch.float32
    x2 = x.reshape(rows, -1).astype(np.float64)
    err = np.abs(y.numpy().reshape(rows, -1) - Y.fir(x2, h.astype(np.float64)))
    assert (err <= Y.bound(x2, h) + np.spacing(np.float32(1e-30))).all()


def test_convolved_bank_normalize_and_gradient():
    rng = np.random.default_rng(5)
    bank = rng.standard_normal((4, 50)).astype(np.float32)
    x = torch.from_numpy(rng.standard_normal((6, 1, 400)).astype(np.float32)).requires_grad_(True)
    att = awm_amd.Convolved(torch.from_numpy(bank), normalize=True, seed=21)
    assert torch.allclose(att.h.double().pow(2).sum(dim=1), torch.ones(4, dtype=torch.float64), atol=1e-6)
    y = att(x, row0=3)
    idx = Y.bank_index(21, 0, 3 + np.arange(6), 4)
    assert att.draw == 1 and np.array_equal(att.last_index.numpy(), idx)
    hn = att.h.numpy().astype(np.float64)[idx]
    x2 = x.detach().numpy().reshape(6, -1).astype(np.float64)
    assert (np.abs(y.detach().numpy().reshape(6, -1) - Y.fir(x2, hn)) <= Y.bound(x2, hn)).all()
    g = rng.standard_normal((6, 1, 400)).astype(np.float32)
    y.backward(torch.from_numpy(g))
    g2 = g.reshape(6, -1).astype(np.float64)
    assert (np.abs(x.grad.numpy().reshape(6, -1) - Y.fir_adjoint(g2, hn)) <= Y.bound_adjoint(g2, hn)).all()
    assert att.h.grad is None and not att.h.requires_grad
    # a split batch draws what the whole batch does
    att.reset()
    whole = att(x.detach())
    att.reset()
    parts = torch.cat([att.reset()(x.detach()[:2]), att.reset()(x.detach()[2:], row0=2)])
    assert torch.equal(whole, parts)
    one = awm_amd.Convolved(torch.tensor([1.0]))(x.detach())
    assert torch.equal(one, x.detach())


@pytest.mark.parametrize("shape", [(3, 1, 600), (2, 350), (200,)])
def test_reverb_cpu_path_against_float64(shape):
    rng = np.random.default_rng(6)
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    x = rng.standard_normal(shape).astype(np.float32)
    att = awm_amd.Reverb(taps=257, seed=8)
    y = att(torch.from_numpy(x), row0=4)
    assert y.shape == x.shape and att.draw == 1
    rt60, drr = Y.reverb_params(8, 0, 4 + np.arange(rows), (0.1, 0.4), (0, 12))
    assert np.array_equal(att.last_params.numpy(), np.stack([rt60, drr], axis=1)) and tuple(att.last_ir.shape) == (rows, 257)
    h64 = np.stack([Y.rir(8, 0, 4 + r, rt60[r], drr[r], 257, 16000.0)[0] for r in range(rows)])
    assert np.abs(att.last_ir.numpy() - h64).max() <= 2.0 ** -24 * np.abs(h64).max()
    h = att.last_ir.numpy().astype(np.float64)
    x2 = x.reshape(rows, -1).astype(np.float64)
    assert (np.abs(y.numpy().reshape(rows, -1) - Y.fir(x2, h)) <= Y.bound(x2, h)).all()
    power = float((y.double() ** 2).mean() / (torch.from_numpy(x).double() ** 2).mean())
    assert 0.5 < power < 2.0, "unit-energy responses keep the power of white input"


def test_reverb_draw_reset_and_row0():
    x = torch.from_numpy(np.random.default_rng(7).standard_normal((5, 300)).astype(np.float32))
    att = awm_amd.Reverb(taps=64, seed=2)
    a, b = att(x), att(x)
    assert att.draw == 2 and not torch.equal(a, b)
    assert torch.equal(att.reset()(x), a) and torch.equal(att.reset(1)(x), b)
    whole_ir = att.reset()(x) is not None and att.last_ir.clone()
    parts = torch.cat([att.reset()(x[:2]), att.reset()(x[2:], row0=2)])
    assert torch.equal(parts, a) and torch.equal(att.last_ir, whole_ir[2:])
    fixed = awm_amd.Reverb(rt60=0.2, drr_db=3, taps=16)
    fixed(x)
    assert (fixed.last_params[:, 0] == np.float32(0.2)).all() and (fixed.last_params[:, 1] == 3).all()


def test_echo_ir():
    h = awm_amd.echo_ir(0.05, -6.0)
    assert h.dtype == torch.float32 and h.shape == (801,), "0.05 s at 16 kHz: the echo sits on tap 800"
    g = 10.0 ** (-6.0 / 20.0)
    assert abs(float(h.double().pow(2).sum()) - 1.0) <= 1e-6 and int((h != 0).sum()) == 2
    assert abs(float(h[800] / h[0]) - g) <= 1e-6
    x = torch.zeros(1, 2000); x[0, 10] = 1.0
    y = awm_amd.Convolved(h)(x)
    assert y[0, 10] == h[0] and y[0, 810] == h[800] and int((y != 0).sum()) == 2
    assert awm_amd.echo_ir(0.001, 0.0, sample_rate=8000).shape == (9,)


def test_argument_errors():
    for kw in (dict(rt60=0), dict(rt60=(-0.1, 0.3)), dict(rt60=(0.4, 0.1)), dict(rt60=True), dict(rt60="long"), dict(rt60=float("nan")),
               dict(rt60=(0.1, 0.2, 0.3)), dict(drr_db=(12, 0)), dict(drr_db=float("inf")), dict(drr_db=False), dict(taps=0),
               dict(taps=16385), dict(taps=2048.0), dict(taps=True), dict(sample_rate=0), dict(sample_rate=True),
               dict(sample_rate=float("nan")), dict(seed=1.5), dict(seed=True)):
        with pytest.raises(ValueError):
            awm_amd.Reverb(**kw)
    att = awm_amd.Reverb(taps=8)
    for bad in (-1, 2 ** 32, 1.0, True):
        with pytest.raises(ValueError):
            att.reset(bad)
    x = torch.zeros(2, 100)
    for bad in (-1, 2 ** 32 - 1, 0.0, True):
        with pytest.raises(ValueError):
            att(x, row0=bad)
    with pytest.raises(ValueError):
        att(torch.zeros(2, 1, 1, 100))
    with pytest.raises(TypeError):
        att([0.0] * 100)
    C = awm_amd.Convolved
    for h in (torch.zeros(0), torch.zeros(2, 3, 4), torch.zeros(16385), torch.tensor([1.0, float("nan")]), [1.0, 0.5], None):
        with pytest.raises(ValueError):
            C(h)
    with pytest.raises(ValueError):
        C(torch.zeros(2, 8), normalize=True)
    for kw in (dict(normalize=1), dict(seed=True), dict(seed=0.5)):
        with pytest.raises(ValueError):
            C(torch.ones(4), **kw)
    for args in ((0.0, -6.0), (2.0, -6.0), (float("nan"), 0.0), (0.01, float("inf")), (0.01, 0.0, 0), (True, 0.0), ("late", 0.0)):
        with pytest.raises(ValueError):
            awm_amd.echo_ir(*args)


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fir_rows(torch.zeros(2, 10), torch.ones(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rir_synth(torch.zeros(2, 2), 16)
    assert "no gradient" in " ".join(ops.FirRowsFn.__doc__.lower().split())


# ------------------------------------------------------------------------------------------ the C boundary
def test_launchers_reject_bad_arguments_without_a_gpu():
    """hipErrorInvalidValue (1) comes back before anything is launched, so these calls need no device"""
    for args in Y.BAD_FIR_ARGS:
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm_amd.lib.wm_fir_rows(*args)
    for args in Y.BAD_RIR_ARGS:
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm_amd.lib.wm_rir_synth(*args)


def test_entry_points_are_declared_and_exported():
    protos = _lib.parse_header()
    assert [name for _, name in protos["wm_fir_rows"]] == ["x", "h", "y", "rows", "n", "K", "h_stride", "reverse", "stream"]
    assert [name for _, name in protos["wm_rir_synth"]] == ["params", "h", "rows", "K", "sample_rate", "row0", "seed", "draw", "stream"]
    assert os.path.exists(_lib.LIB_PATH), "build with __graft_entry__.build()"
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("wm_fir_rows", "wm_rir_synth"):
        assert hasattr(dll, name), f"{name} declared in include/wm_hip.h but not exported"
    for name in ("Convolved", "Reverb", "echo_ir"):
        assert name in awm_amd.__all__ and hasattr(awm_amd, name)
