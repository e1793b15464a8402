"""The pitch-preserving time stretch without a GPU: the draws (words o1 and o2 of the warp_phase counter) and the window against the
float64 yardstick of tests/wsola_yardstick.py, the CPU path of attacks.TimeStretch / attacks.PitchShift -- identity, the exact integer
search, synthesis within the fmaf bound, autograd against the dense matrix --, argument validation, and the C boundary (the launcher
refuses bad arguments before any launch, so those calls need no device)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import awm_amd
from awm_amd import _lib, attacks, ops

import draw_yardstick as D
import time_warp_yardstick as TW
import wsola_yardstick as Y


# ------------------------------------------------------------------------------------------ draws and counters
def test_draws_are_words_o1_and_o2_of_the_warp_phase_counter():
    seed, draw, rows = (5 << 32) + 9, 3, np.arange(7, 40)
    r = attacks.row_stretch_rates(seed, draw, rows, (0.8, 1.25))
    assert r.dtype == np.float32 and r.shape == (33,) and np.array_equal(r, Y.stretch_rates(seed, draw, rows, (0.8, 1.25)))
    assert (r >= np.float32(0.8)).all() and (r <= np.float32(1.25)).all() and r.std() > 0.05 and len(set(r)) == 33
    assert not np.array_equal(r, attacks.row_stretch_rates(seed, draw + 1, rows, (0.8, 1.25)))
    assert not np.array_equal(r, attacks.row_stretch_rates(seed + 1, draw, rows, (0.8, 1.25)))
    assert (attacks.row_stretch_rates(seed, draw, rows, (1.1, 1.1)) == np.float32(1.1)).all()
    st, beta, rate = attacks.row_pitch_params(seed, draw, rows, (-3, 4))
    want = Y.pitch_params(seed, draw, rows, (-3, 4))
    for got, ref in zip((st, beta, rate), want):
        assert got.dtype == np.float32 and np.array_equal(got, ref)
    assert (st >= -3).all() and (st <= 4).all() and np.allclose(beta, 2.0 ** (st / 12.0), rtol=1e-6) and np.allclose(rate * beta, 1, rtol=1e-6)
    # the words: o0 stays TimeWarp's flutter phase, o1 and o2 are the new draws, and the three differ
    o = D.philox4x32_10((*D.WARP_PHASE, rows, draw), D.key_of(seed))
    phase = attacks.row_warp_params(seed, draw, rows, (1.0, 1.0), (0.0, 0.0), (4.0, 4.0), (0.1, 0.1), 16000)[:, 4]
    assert np.array_equal(phase, D.unit(o[0]).astype(np.float32))
    assert np.array_equal(r, D.affine32((0.8, 1.25), D.unit(o[1]))) and np.array_equal(st, D.affine32((-3, 4), D.unit(o[2])))
    assert not np.array_equal(o[0], o[1]) and not np.array_equal(o[1], o[2])


def test_families_are_unchanged():
    fixed = {name: f for name, f in attacks.FAMILIES.items() if f[0] is not None}
    assert fixed == D.FAMILIES and len(attacks.FAMILIES) == 6 + 2 * ops.SPLICE_MAX_SPANS
    assert attacks.FAMILIES["warp_phase"] == D.WARP_PHASE == (0xFFFFFFFC, 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------ the window
@pytest.mark.parametrize("L", [64, 256, 512, 1024])
def test_window_against_the_yardstick(L):
    w = ops.wsola_window(L)
    assert w.dtype == torch.float32 and tuple(w.shape) == (L // 2,) and not w.is_cuda and ops.wsola_window(L) is w, "cached"
    ref = Y.window(L)
    assert (np.abs(w.numpy() - ref) <= np.spacing(np.abs(ref))).all() and w[0] == 0.0 and w[L // 4] == 0.5
    assert (np.diff(w.numpy()) > 0).all() and w[-1] < 1.0
    assert ops.wsola_frames(1000, L) == Y.frames(1000, L) and ops.wsola_frames(L, L) == 3


def test_dims_refusals():
    for L, S in ((32, 16), (2048, 128), (500, 100), (512, 0), (512, 257), (512.0, 128), (True, 1), (512, True), (512, 1.0)):
        with pytest.raises(ValueError):
            ops._wsola_dims(L, S)
    for L in (32, 2048, 100, 64.0):
        with pytest.raises(ValueError):
            ops.wsola_window(L)


# ------------------------------------------------------------------------------------------ the CPU path
def _host(x, rates, n_out, L, S):
    y, delta = attacks._wsola_rows_host(torch.from_numpy(x), np.asarray(rates, dtype=np.float32), n_out, L, S)
    return y.numpy(), delta.numpy()


@pytest.mark.parametrize("L,S", Y.DIMS)
@pytest.mark.parametrize("n", [1, 63, 257, 1000])
def test_cpu_identity_bit_for_bit(n, L, S):
    x = np.random.default_rng(n).standard_normal((3, n)).astype(np.float32)
    x[1, n // 3:n // 2] = 0.0                                # a silent stretch
    x[2] = 0.0
    for n_out in (n, n + 70, max(1, n - 40)):
        y, delta = _host(x, [1.0] * 3, n_out, L, S)
        want = np.zeros((3, n_out), dtype=np.float32)
        want[:, :min(n, n_out)] = x[:, :min(n, n_out)]
        assert np.array_equal(y.view(np.int32), want.view(np.int32)) and not delta.any() and delta.shape == (3, Y.frames(n_out, L))


@pytest.mark.parametrize("L,S", Y.DIMS)
@pytest.mark.parametrize("n", [63, 257, 1000])
def test_cpu_integer_search_is_exact_and_synthesis_within_the_bound(n, L, S):
    x = Y.integer_rows(n, 100 * n + L)
    for rate in Y.RATES:
        y, delta = _host(x, [rate, rate], n, L, S)
        for r in range(2):
            want = Y.search(x[r], rate, n, L, S)
            assert np.array_equal(delta[r], want), f"n {n} ({L}, {S}) rate {rate} row {r}: first at frame {np.argmax(delta[r] != want)}"
            ref, bnd = Y.synth(x[r], rate, want, n, L, S)
            assert (np.abs(y[r] - ref) <= bnd).all()


def test_cpu_garbage_rate_rows_are_zeros():
    x = np.random.default_rng(3).standard_normal((3, 300)).astype(np.float32)
    for g in Y.GARBAGE_RATES + (0.2, 4.5):
        y, delta = _host(x, [0.8, g, 1.25], 300, 64, 16)
        assert not y[1].any() and not delta[1].any() and y[0].any() and y[2].any()


@pytest.mark.parametrize("rate", [0.8, 1.0, 1.25])
def test_autograd_gradient_is_the_transposed_matrix(rate):
    n, L, S = 300, 64, 16
    rng = np.random.default_rng(6)
    x = torch.from_numpy(Y.speech_rows(2, n, 5)).requires_grad_(True)
    g = rng.standard_normal((2, n)).astype(np.float32)
    att = awm_amd.TimeStretch(rate=rate, frame=L, search=S)
    y = att(x)
    y.backward(torch.from_numpy(g))
    delta = att.last_delta.numpy()
    assert delta.dtype == np.int32 and delta.shape == (2, Y.frames(n, L)) and (rate == 1.0 or delta.any())
    for r in range(2):
        M = Y.matrix(rate, delta[r], n, n, L, S)
        ref, bnd = Y.adjoint(g[r], rate, delta[r], n, L, S)
        assert np.abs(M.T @ g[r].astype(np.float64) - ref).max() <= 1e-12, "the yardstick's adjoint is its dense matrix transposed"
        y64, ybnd = Y.synth(x.detach().numpy()[r], rate, delta[r], n, L, S)
        assert np.abs(M @ x.detach().numpy()[r].astype(np.float64) - y64).max() <= 1e-12
        assert (np.abs(y.detach().numpy()[r] - y64) <= ybnd).all()
        err = np.abs(x.grad.numpy()[r].astype(np.float64) - ref)
        assert (err <= bnd + 1e-300).all() and np.abs(ref).max() > 0.1
        assert not Y.check_search(x.detach().numpy()[r], rate, delta[r], n, L, S)[1]


# ------------------------------------------------------------------------------------------ the modules
def test_time_stretch_module_draws_and_rewinds():
    x = torch.from_numpy(Y.speech_rows(5, 700, 9))
    att = awm_amd.TimeStretch(rate=(0.8, 1.25), frame=256, search=64, seed=2)
    a, b = att(x, row0=4), att(x, row0=4)
    assert a.shape == x.shape and a.dtype == torch.float32 and att.draw == 2 and not torch.equal(a, b)
    assert np.array_equal(att.last_params.numpy(), Y.stretch_rates(2, 1, 4 + np.arange(5), (0.8, 1.25))) and not att.last_params.is_cuda
    assert torch.equal(att.reset()(x, row0=4), a) and torch.equal(att.reset(1)(x, row0=4), b)
    whole, wd = att.reset()(x), att.last_delta.clone()
    parts = torch.cat([att.reset()(x[:2]), att.reset()(x[2:], row0=2)])
    assert torch.equal(parts, whole) and torch.equal(att.last_delta, wd[2:]), "a batch cut into pieces draws what the whole batch does"
    assert "rate=(0.8, 1.25)" in repr(att) and "search=64" in repr(att)
    for shape in ((2, 1, 300), (300,)):
        z = awm_amd.TimeStretch(rate=1.0)(torch.ones(shape))
        assert z.shape == shape and torch.equal(z, torch.ones(shape))
    doc = " ".join(awm_amd.TimeStretch.__doc__.split())
    assert "labels are not moved" in doc.lower() and "UNMEASURED" in doc and "constants of the graph" in " ".join(ops.WsolaFn.__doc__.lower().split())


def test_pitch_shift_module_is_the_chain_of_its_two_maps():
    n = 900
    x = torch.from_numpy(Y.speech_rows(3, n, 11)).reshape(3, 1, n)
    att = awm_amd.PitchShift(semitones=(-4, 4), frame=256, search=64, seed=5)
    y = att(x, row0=2)
    st, beta, rate = Y.pitch_params(5, 0, 2 + np.arange(3), (-4, 4))
    assert y.shape == x.shape and np.array_equal(att.last_params.numpy(), np.stack([st, beta, rate], axis=1))
    for r in range(3):
        m = max(n, int(np.ceil(float(beta[r]) * n)))
        z, delta = attacks._wsola_rows_host(x[r], rate[r:r + 1], m, 256, 64)
        prm = np.array([[beta[r], 0, 0, 0, 0, min(1.0, 1.0 / float(beta[r]))]], dtype=np.float32)
        want = attacks._warp_rows_host(z, torch.from_numpy(prm), ops.time_warp_table(), 16, 512)[:, :n]
        assert torch.equal(y[r], want), f"row {r}: the batch equals the row on its own, cut at its own m = {m}"
        assert np.array_equal(att.last_delta[r, :delta.shape[1]].numpy(), delta[0])
        ref, bnd = TW.forward(z.numpy(), prm, TW.table())
        assert (np.abs(y[r].numpy() - ref[:, :n]) <= bnd[:, :n]).all()
    whole = att.reset()(x)
    parts = torch.cat([att.reset()(x[:1]), att.reset()(x[1:], row0=1)])
    assert torch.equal(whole, parts)
    zero = awm_amd.PitchShift(semitones=0.0)(x)
    assert torch.equal(zero, x), "no shift: rate 1 and speed 1 hand the samples on bit for bit"
    xg = x.clone().requires_grad_(True)
    att.reset()(xg).square().sum().backward()
    assert bool(torch.isfinite(xg.grad).all()) and bool((xg.grad != 0).any())


def test_constructor_and_forward_refusals():
    for T, name, lo, hi in ((awm_amd.TimeStretch, "rate", 0.5, 2.0), (awm_amd.PitchShift, "semitones", -12.0, 12.0)):
        for v in (lo - 0.01, hi + 0.01, (lo - 1, 1.0), (hi, lo), True, "fast", float("nan"), (1.0, 1.0, 1.0)):
            with pytest.raises(ValueError):
                T(**{name: v})
        for kw in (dict(frame=500), dict(frame=32), dict(frame=2048), dict(frame=512.0), dict(search=0), dict(search=257), dict(search=True),
                   dict(frame=64, search=33), dict(seed=1.5), dict(seed=True)):
            with pytest.raises(ValueError):
                T(**kw)
        T(**{name: lo}), T(**{name: hi}), T(frame=64, search=32), T(frame=1024, search=512)
        att = T()
        for bad in (-1, 2 ** 32, 1.0, True):
            with pytest.raises(ValueError):
                att.reset(bad)
        for bad in (-1, 2 ** 32 - 1, 0.0, True):
            with pytest.raises(ValueError):
                att(torch.zeros(2, 100), row0=bad)
        with pytest.raises(ValueError):
            att(torch.zeros(2, 1, 1, 100))
        with pytest.raises(TypeError):
            att([0.0] * 100)
        assert att.draw == 0, "a call that raises consumes no draw"
    for kw in (dict(zeros=3), dict(zeros=33), dict(zeros=16.0)):
        with pytest.raises(ValueError):
            awm_amd.PitchShift(**kw)


def test_ops_refuse_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.wsola(torch.zeros(2, 100), torch.ones(2))


def test_inside_sequential_with_the_pcm_codec():
    x = 0.1 * torch.from_numpy(Y.speech_rows(2, 600, 10)).reshape(2, 1, 600)
    chain = torch.nn.Sequential(awm_amd.TimeStretch(rate=1.1, frame=256, search=64), awm_amd.PitchShift(semitones=1.0, frame=256, search=64),
                                awm_amd.PcmCodec())
    y = chain(x)
    assert y.shape == x.shape and bool(torch.isfinite(y).all()) and chain[0].draw == 1 and chain[1].draw == 1
    want = awm_amd.PcmCodec()(awm_amd.PitchShift(semitones=1.0, frame=256, search=64)(awm_amd.TimeStretch(rate=1.1, frame=256, search=64)(x)))
    assert torch.equal(y, want)


# ------------------------------------------------------------------------------------------ the interface and the build
def test_launcher_rejects_bad_arguments_without_a_gpu():
    """hipErrorInvalidValue (1) comes back before anything is launched, so these calls need no device"""
    for args in Y.BAD_ARGS:
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm_amd.lib.wm_wsola(*args)


def test_entry_point_is_declared_exported_and_built():
    protos = _lib.parse_header()
    assert [name for _, name in protos["wm_wsola"]] == ["x", "rate", "win", "y", "delta", "rows", "n_in", "n_out", "L", "S", "mode", "stream"]
    assert [c for c, _ in protos["wm_wsola"]][:5] == ["const float*", "const float*", "const float*", "float*", "int*"]
    assert os.path.exists(_lib.LIB_PATH), "build with __graft_entry__.build()"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "wm_wsola"), "wm_wsola declared in include/wm_hip.h but not exported"
    for name in ("TimeStretch", "PitchShift"):
        assert name in awm_amd.__all__ and getattr(awm_amd, name) is getattr(attacks, name)
    build = open(os.path.join(_lib._PKG_DIR, "csrc", "build.sh")).read()
    assert "wsola" in build.split("for f in")[1].split(";")[0].split()
    assert os.path.exists(os.path.join(_lib._PKG_DIR, "csrc", "wsola.hip"))
