"""The speed-change / wow-and-flutter attack without a GPU: the draws (attacks.row_warp_params) and the table (ops.time_warp_table) against
the float64 yardstick of tests/time_warp_yardstick.py, the Philox counter domains, the CPU path of attacks.TimeWarp and its autograd
gradient, argument validation, and the C boundary (the launcher refuses bad arguments before any launch, so those calls need no device)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import awm_amd
from awm_amd import _lib, attacks, ops

import draw_yardstick as D
import time_warp_yardstick as Y

MODULES = [dict(), dict(speed=0.8), dict(speed=1.25, shift_s=0.004), dict(speed=2.0, shift_s=-0.002),
           dict(speed=(0.9, 1.1), flutter_hz=4.0, flutter_depth=0.01), dict(speed=1.0, flutter_hz=(0.5, 8.0), flutter_depth=(0.05, 0.25))]


def _draw(att, rows, row0=0, draw=0):
    return Y.warp_params(att.seed, draw, row0 + np.arange(rows), att.speed, att.shift_s, att.flutter_hz, att.flutter_depth,
                         float(att.sample_rate))


# ------------------------------------------------------------------------------------------ draws and counters
def test_draws_are_reproducible_and_the_yardsticks():
    seed, draw, rows = (5 << 32) + 9, 3, np.arange(7, 40)
    args = ((0.9, 1.1), (-0.01, 0.02), (0.5, 8.0), (0.0, 0.25), 16000)
    p = attacks.row_warp_params(seed, draw, rows, *args)
    assert p.dtype == np.float32 and p.shape == (33, 6)
    assert np.array_equal(p, attacks.row_warp_params(seed, draw, rows, *args)), "reproducible"
    assert np.array_equal(p, Y.warp_params(seed, draw, rows, *args[:4], 16000.0)), "the package's draws are the yardstick's"
    assert not np.array_equal(p, attacks.row_warp_params(seed, draw + 1, rows, *args))
    assert not np.array_equal(p, attacks.row_warp_params(seed + 1, draw, rows, *args))
    a, off, d, w, phi, c = p.T.astype(np.float64)
    assert (a >= np.float32(0.9)).all() and (a <= np.float32(1.1)).all() and a.std() > 0.02
    assert (off >= -160.0).all() and (off <= 320.0).all() and (w > 0).all() and (w <= 8.0 / 16000 * (1 + 1e-6)).all()
    assert (phi > 0).all() and (phi < 1).all() and len(set(phi)) == 33
    depth = 2 * np.pi * w * np.abs(d) / a
    assert (depth <= 0.25 * (1 + 1e-6)).all(), "the instantaneous speed a (1 + depth cos) stays positive: p is strictly increasing"
    assert (c <= 1).all() and (c >= 0.4 / 1.1).all() and np.allclose(c, np.minimum(1, 1 / (a * (1 + depth))), rtol=1e-6)
    fixed = attacks.row_warp_params(seed, draw, rows, (1.05, 1.05), (0.0, 0.0), None, None, 16000)
    assert (fixed[:, 0] == np.float32(1.05)).all() and not fixed[:, 1:5].any() and (fixed[:, 5] == np.float32(1 / np.float64(np.float32(1.05)))).all()
    assert np.array_equal(fixed, Y.warp_params(seed, draw, rows, (1.05, 1.05), (0.0, 0.0), None, None))


def test_the_new_counters_meet_none_of_the_others():
    """(word 0, word 1) of every family for one (seed, draw, row), from the package's table and from the yardstick's: samples (q, 0), a
    response's taps (k >> 2, ~0 - 1), the four parameter counters (~0 - i, ~0), i = 0..3, and Splice's sixteen (~0 - 4 - i, ~0), i = 0..15"""
    assert attacks.FAMILIES["param"] == Y.PARAM == (0xFFFFFFFF, 0xFFFFFFFF)
    assert attacks.FAMILIES["param2"] == Y.PARAM2 == (0xFFFFFFFE, 0xFFFFFFFF)
    assert attacks.FAMILIES["warp"] == Y.WARP == (0xFFFFFFFD, 0xFFFFFFFF)
    assert attacks.FAMILIES["warp_phase"] == Y.WARP_PHASE == (0xFFFFFFFC, 0xFFFFFFFF)
    assert attacks.FAMILIES["sample"] == (None, D.SAMPLE_HIGH) and attacks.FAMILIES["rir_tap"] == (None, Y.RIR_HIGH)
    fixed = {name: f for name, f in attacks.FAMILIES.items() if f[0] is not None}
    assert fixed == D.FAMILIES and len(fixed) == len(attacks.FAMILIES) - 2 == 4 + 2 * ops.SPLICE_MAX_SPANS
    assert [fixed[f"splice_span{j}"][0] for j in range(8)] == [0xFFFFFFFB - 2 * j for j in range(8)]
    assert [fixed[f"splice_shift{j}"][0] for j in range(8)] == [0xFFFFFFFA - 2 * j for j in range(8)]
    families = list(fixed.values())
    assert families[:4] == [Y.PARAM, Y.PARAM2, Y.WARP, Y.WARP_PHASE]
    assert len({f[0] for f in families}) == len(families) == 20, "all first words are distinct"
    q_max, k_max = (1 << 34) - 1 >> 2, ops.FIR_MAX_TAPS - 1 >> 2
    for f in families:
        assert f[1] != 0 and f[1] != Y.RIR_HIGH, "a sample counter's high word is 0, a tap counter's 0xFFFFFFFE"
    assert q_max >> 32 == 0 and k_max < min(f[0] for f in families) == 0xFFFFFFEC
    key = Y.key_of(12345)
    words = [tuple(Y.philox4x32_10((c0, c1, 9, 2), key).tolist()) for c0, c1 in [(0, 0), (0, Y.RIR_HIGH)] + families]
    assert len(set(words)) == 22, "and the numbers differ"
    for name, f in fixed.items():
        assert np.array_equal(attacks._words(name, 12345, 2, 9), Y.philox4x32_10((*f, 9, 2), key)), name
    # the reverb's draws are what they were
    rt60, _ = attacks.row_reverb_params(12345, 2, np.array([9]), (0.1, 0.4), (0, 12))
    u = Y.unit(Y.philox4x32_10((*Y.PARAM2, 9, 2), key)[0])
    assert rt60[0] == np.float32(np.float64(np.float32(0.4) - np.float32(0.1)) * u + np.float64(np.float32(0.1)))


def test_a_cut_batch_draws_what_the_whole_batch_draws():
    x = torch.from_numpy(np.random.default_rng(7).standard_normal((5, 300)).astype(np.float32))
    att = awm_amd.TimeWarp(speed=(0.8, 1.25), shift_s=(-0.001, 0.001), flutter_hz=(2.0, 6.0), flutter_depth=(0.0, 0.1), seed=2)
    a, b = att(x), att(x)
    assert att.draw == 2 and not torch.equal(a, b)
    assert torch.equal(att.reset()(x), a) and torch.equal(att.reset(1)(x), b)
    att.reset()(x)
    whole = att.last_params.clone()
    assert not whole.is_cuda and np.array_equal(whole.numpy(), _draw(att, 5))
    parts = torch.cat([att.reset()(x[:2]), att.reset()(x[2:], row0=2)])
    assert torch.equal(parts, a) and torch.equal(att.last_params, whole[2:])
    assert "speed=(0.8, 1.25)" in repr(att) and "flutter_depth=(0.0, 0.1)" in repr(att)


# ------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("zeros,res", [(16, 512), (8, 64), (4, 1024), (32, 512)])
def test_table_against_the_yardstick(zeros, res):
    tab = ops.time_warp_table(zeros, res)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (zeros * res + 2,) and not tab.is_cuda
    assert ops.time_warp_table(zeros, res) is tab, "cached"
    t, ref = tab.numpy(), Y.table(zeros, res)
    assert (np.abs(t - ref) <= np.spacing(np.abs(ref))).all(), "within one float32 ulp"
    assert t[0] == 1.0 and not t[res::res].any() and not t[-2:].any(), "the pinned entries are exact"
    assert (np.abs(t[1:res]) > 0).all() and abs(t[res // 2] - 2 / np.pi * 0.5 * (1 + np.cos(np.pi / (2 * zeros)))) < 1e-6


def test_table_and_dims_refusals():
    for z, r in ((3, 512), (33, 512), (16, 32), (16, 2048), (16, 500), (32, 1024), (16.0, 512), (True, 512), (16, True)):
        with pytest.raises(ValueError):
            ops.time_warp_table(z, r)


# ------------------------------------------------------------------------------------------ refusals
def test_constructor_and_forward_refusals():
    T = awm_amd.TimeWarp
    for kw in (dict(speed=0.49), dict(speed=2.01), dict(speed=(0.4, 1.0)), dict(speed=(1.1, 0.9)), dict(speed=True), dict(speed="fast"),
               dict(speed=float("nan")), dict(speed=(0.9, 1.0, 1.1)), dict(shift_s=float("inf")), dict(shift_s=float("nan")),
               dict(shift_s=(0.1, 0.0)), dict(flutter_hz=4.0), dict(flutter_depth=0.1), dict(flutter_hz=0.0, flutter_depth=0.1),
               dict(flutter_hz=-1.0, flutter_depth=0.1), dict(flutter_hz=4000.5, flutter_depth=0.1), dict(flutter_hz=4.0, flutter_depth=0.26),
               dict(flutter_hz=4.0, flutter_depth=-0.01), dict(flutter_hz=4.0, flutter_depth=(0.2, 0.3)), dict(zeros=3), dict(zeros=33),
               dict(zeros=16.0), dict(zeros=True), dict(sample_rate=0), dict(sample_rate=True), dict(sample_rate=float("nan")),
               dict(seed=1.5), dict(seed=True)):
        with pytest.raises(ValueError):
            T(**kw)
    T(speed=0.5), T(speed=2), T(flutter_hz=4000.0, flutter_depth=0.25), T(flutter_hz=2000.0, flutter_depth=0.0, sample_rate=8000)
    att = T()
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


def test_ops_refuse_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.time_warp(torch.zeros(2, 10), torch.zeros(2, 6))
    assert "constants of the graph" in " ".join(ops.TimeWarpFn.__doc__.lower().split())
    doc = " ".join(awm_amd.TimeWarp.__doc__.split())
    assert "silence" in doc and "labels are not moved" in doc.lower() and "UNMEASURED" in doc


# ------------------------------------------------------------------------------------------ the CPU path
@pytest.mark.parametrize("kw", MODULES)
@pytest.mark.parametrize("shape", [(3, 1, 700), (2, 450), (257,)])
def test_cpu_path_against_float64(kw, shape):
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    x = np.random.default_rng(4).standard_normal(shape).astype(np.float32)
    att = awm_amd.TimeWarp(seed=8, **kw)
    y = att(torch.from_numpy(x), row0=4)
    assert y.shape == x.shape and y.dtype == torch.float32 and att.draw == 1
    params = _draw(att, rows, row0=4)
    assert np.array_equal(att.last_params.numpy(), params)
    ref, bnd = Y.forward(x.reshape(rows, -1), params, Y.table())
    err = np.abs(y.numpy().reshape(rows, -1).astype(np.float64) - ref)
    print(f"{kw} {shape}: worst err / bound {(err / np.maximum(bnd, 1e-300)).max():.4f}")
    assert (err <= bnd).all()
    assert np.abs(ref).max() > 0.1


def test_cpu_path_with_eight_zero_crossings():
    x = np.random.default_rng(5).standard_normal((2, 500)).astype(np.float32)
    att = awm_amd.TimeWarp(speed=1.1, zeros=8, seed=1)
    y = att(torch.from_numpy(x))
    ref, bnd = Y.forward(x, _draw(att, 2), Y.table(8, 512), 8, 512)
    assert (np.abs(y.numpy() - ref) <= bnd).all()


@pytest.mark.parametrize("kw", MODULES)
def test_autograd_gradient_is_the_transposed_matrix(kw):
    n = 257
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.standard_normal((2, n)).astype(np.float32)).requires_grad_(True)
    g = rng.standard_normal((2, n)).astype(np.float32)
    att = awm_amd.TimeWarp(seed=3, **kw)
    att(x).backward(torch.from_numpy(g))
    params = _draw(att, 2)
    ref, bnd = Y.adjoint(g, params, Y.table())
    for r in range(2):
        M = Y.matrix(params[r], n, Y.table())
        assert np.abs(M.T @ g[r].astype(np.float64) - ref[r]).max() <= 1e-12, "the yardstick's adjoint is its dense matrix transposed"
        assert np.abs(M @ x.detach().numpy()[r].astype(np.float64) - Y.forward(x.detach().numpy(), params, Y.table())[0][r]).max() <= 1e-12
    err = np.abs(x.grad.numpy().astype(np.float64) - ref)
    print(f"{kw}: gradient worst err / bound {(err / np.maximum(bnd, 1e-300)).max():.4f}")
    assert (err <= bnd).all() and np.abs(ref).max() > 0.1


@pytest.mark.parametrize("shift", [0, 5, -3, 350, -350])
def test_speed_one_is_a_shift_bit_for_bit(shift):
    n = 300
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((2, n)).astype(np.float32))
    y = awm_amd.TimeWarp(speed=1.0, shift_s=shift / 16000)(x)
    want = torch.zeros_like(x)
    lo, hi = max(0, -shift), min(n, n - shift)
    if lo < hi:
        want[:, lo:hi] = x[:, lo + shift:hi + shift]
    assert torch.equal(y, want), "whole-sample shifts hand the samples on unchanged, zeros where the shift leaves the row"


def test_inside_sequential_with_the_pcm_codec():
    """on the CPU the codec is forward only: the chain's gradient is the GPU test's"""
    x = 0.1 * torch.from_numpy(np.random.default_rng(10).standard_normal((2, 1, 600)).astype(np.float32))
    chain = torch.nn.Sequential(awm_amd.TimeWarp(speed=1.05), awm_amd.PcmCodec())
    y = chain(x)
    assert y.shape == x.shape and bool(torch.isfinite(y).all()) and chain[0].draw == 1
    warped = awm_amd.TimeWarp(speed=1.05)(x)
    assert torch.equal(y, awm_amd.PcmCodec()(warped)) and not torch.equal(y, warped)
    grid = y.double() * 32767
    assert float((grid - grid.round()).abs().max()) < 1e-2, "the chain ends on the 16-bit grid"


# ------------------------------------------------------------------------------------------ the interface and the build
def test_launcher_rejects_bad_arguments_without_a_gpu():
    """hipErrorInvalidValue (1) comes back before anything is launched, so these calls need no device"""
    for args in Y.BAD_ARGS:
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm_amd.lib.wm_time_warp(*args)


def test_entry_point_is_declared_exported_and_built():
    protos = _lib.parse_header()
    assert [name for _, name in protos["wm_time_warp"]] == ["x", "params", "tab", "y", "rows", "n", "zeros", "res", "adjoint", "stream"]
    assert os.path.exists(_lib.LIB_PATH), "build with __graft_entry__.build()"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "wm_time_warp"), "wm_time_warp declared in include/wm_hip.h but not exported"
    assert "TimeWarp" in awm_amd.__all__ and awm_amd.TimeWarp is attacks.TimeWarp
    build = open(os.path.join(_lib._PKG_DIR, "csrc", "build.sh")).read()
    assert "time_warp" in build.split("for f in")[1].split(";")[0].split()
    assert os.path.exists(os.path.join(_lib._PKG_DIR, "csrc", "time_warp.hip"))
