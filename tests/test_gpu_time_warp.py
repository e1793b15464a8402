"""wm_time_warp / ops.time_warp / ops.TimeWarpFn / attacks.TimeWarp on the GPU against the float64 yardstick of
tests/time_warp_yardstick.py (numpy from the definition in include/wm_hip.h; nothing from the package).  Kernel-level cases use the
yardstick's table and parameter rows: n in Y.NS (one sample, less than a wave, one below / at / above the tile of 256 samples, several tiles,
16000), every speed in {0.5, 0.8, 1, 1.25, 2} times every offset in {0, -7.3, 100.5, n + 50, -n - 50} (the last two leave the row: at
speed <= 1 every sample is silence), flutter off, (4 Hz, 0.01) and (0.5 Hz, 0.25) at the phases the yardstick names, three rows a launch, x and y one float into their buffers.

Tolerances (none tuned to the kernel):
  shifts     a = 1, integer off, d = 0, c = 1: bit for bit.
  floats     |y - y64| <= gamma(T + 4) sum_k |W x_k| + Lip eps_p sum_{k in support} |x_k|  (the yardstick's docstring derives it), for the forward
             map and, summed over t, for the adjoint.
  adjoint    |<W u, v> - <u, W^T v>| <= sum |v| bound(u) + sum |u| bound^T(v), the two bounds carried through the inner products.
Every reference is computed once per case (lru_cache in the yardstick) and never written to.

Measured on an MI355X (largest err / bound per test, printed by every case): see DESIGN.md section 4i."""
import os

import numpy as np
import pytest
import torch

from oracle import wm_oracle as O

import time_warp_yardstick as Y
from gpu_support import awm, dev  # noqa: F401
from gpu_support import bits, reference_models, to_dev

pytestmark = pytest.mark.gpu


def off_by_one_float(a, dev):
    """the same values in a buffer that starts 4 bytes earlier: the returned tensor's pointer is 4 (mod 8)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
    buf[1:] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[1:].view(a.shape)


def launch(dev, x, params, adjoint=False, tab=None):
    """x (R, n), params (R, 6) numpy: launches of three rows (the last one padded with its first rows), x offset by 4 bytes"""
    from awm_amd import ops
    tab = to_dev(Y.table(), dev) if tab is None else tab
    out = []
    for r0 in range(0, len(x), 3):
        idx = [(r0 + i) % len(x) for i in range(3)]
        y = ops.time_warp(off_by_one_float(x[idx], dev), to_dev(params[idx], dev), tab, adjoint=adjoint)
        out.append(y.cpu().numpy()[:min(3, len(x) - r0)])
    return np.concatenate(out)


def shifted(x, s):
    n = x.shape[-1]
    want = torch.zeros_like(x)
    lo, hi = max(0, -s), min(n, n - s)
    if lo < hi:
        want[..., lo:hi] = x[..., lo + s:hi + s]
    return want


# ------------------------------------------------------------------------------------------ 1. whole-sample shifts, bit for bit
@pytest.mark.parametrize("n", Y.NS)
def test_whole_sample_shifts_bit_for_bit(awm, dev, n):
    from awm_amd import ops
    x = off_by_one_float(np.random.default_rng(n).standard_normal((3, n)), dev)
    assert x.data_ptr() % 8 == 4 and (x != 0).all()
    tab = to_dev(Y.table(), dev)
    for s0 in (0, 5, -3, n + 50, -n - 50):
        params = torch.tensor([[1.0, s0, 0, 0, 0, 1], [1.0, s0 + 1, 0, 0, 0, 1.5], [1.0, s0 - 2, 0, 0.25, 0.5, float("nan")]], device=dev)
        y, dx = ops.time_warp(x, params, tab), ops.time_warp(x, params, tab, adjoint=True)
        for r, s in enumerate((s0, s0 + 1, s0 - 2)):
            assert torch.equal(bits(y[r]), bits(shifted(x[r], s))), f"n {n}: forward, shift {s}"
            assert torch.equal(bits(dx[r]), bits(shifted(x[r], -s))), f"n {n}: adjoint, shift {s}"
    assert torch.equal(bits(ops.time_warp(x, params)), bits(y)), "the package's table has the pinned entries too"


# ------------------------------------------------------------------------------------------ 2. floats against float64
@pytest.mark.parametrize("fi", range(len(Y.FLUTTERS)))
@pytest.mark.parametrize("n", Y.NS)
def test_forward_and_adjoint_against_float64(awm, dev, n, fi):
    x, params = Y.case(n, fi)
    for adj in (False, True):
        ref, bnd = Y.case_ref(n, fi, adj)
        y = launch(dev, x, params, adj).astype(np.float64)
        assert y.shape == x.shape
        err = np.abs(y - ref)
        ratio = float((err / np.maximum(bnd, 1e-300)).max()) if (bnd > 0).any() else 0.0
        print(f"n {n} flutter {Y.FLUTTERS[fi]} adjoint {adj}: worst err / bound {ratio:.4f}")
        bad = np.argwhere(err > bnd)
        assert not len(bad), f"n {n} flutter {Y.FLUTTERS[fi]} adjoint {adj}: err / bound {ratio:.3f}, first at {bad[:3].tolist()}, params {params[bad[0][0]]}"
        if n >= 257:
            assert np.abs(ref).max() > 0.1


# ------------------------------------------------------------------------------------------ 3. independent rows, reproducible launches
GARBAGE = ((float("nan"),) * 6, (float("inf"), 0, 0, 0, 0, 1), (float("-inf"), float("inf"), float("nan"), 1, 1, 0), (-1, 0, 0, 0, 0, 0),
           (1e-30, 0, 0, 0, 0, 0), (1, 1e30, 3e38, 3e38, 3e38, 1), (1e30, -1e30, -5, 1e-20, -3e38, 7))


@pytest.mark.parametrize("n", [33, 257, 4099])
def test_rows_are_independent_and_launches_reproducible(awm, dev, n):
    from awm_amd import ops
    x64, p64 = Y.case(n, 1)
    pick = [6, 12, 15]                                   # (speed, offset) = (0.8, -7.3), (1, 100.5), (1.25, 0) of the case's 25 rows
    x, params, tab = to_dev(x64[pick], dev), to_dev(p64[pick], dev), to_dev(Y.table(), dev)
    for adj in (False, True):
        y = ops.time_warp(x, params, tab, adjoint=adj)
        assert torch.equal(bits(ops.time_warp(x, params, tab, adjoint=adj)), bits(y)), "two launches give identical bits"
        for r in range(3):
            one = ops.time_warp(x[r:r + 1].clone(), params[r:r + 1].clone(), tab, adjoint=adj)
            assert torch.equal(bits(one[0]), bits(y[r])), f"row {r} alone equals row {r} of the batch"
        xn = x.clone()
        xn[1] = float("nan")
        yn = ops.time_warp(xn, params, tab, adjoint=adj)
        assert torch.equal(bits(yn[0]), bits(y[0])) and torch.equal(bits(yn[2]), bits(y[2])), "a row of NaN leaves its neighbours as they were"
        # one guard sample on each side of y, and one row of garbage parameters in the middle
        for g in ((params[1].tolist(),) + GARBAGE):
            pg = params.clone()
            pg[1] = torch.tensor(g, device=dev)
            buf = torch.full((3 * n + 2,), 12345.0, device=dev)
            awm.lib.wm_time_warp(x.data_ptr(), pg.data_ptr(), tab.data_ptr(), buf.data_ptr() + 4, 3, n, Y.ZEROS, Y.RES, int(adj),
                                 torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert float(buf[0]) == 12345.0 and float(buf[-1]) == 12345.0, f"guards, params {g}"
            out = buf[1:-1].view(3, n)
            assert torch.equal(bits(out[0]), bits(y[0])) and torch.equal(bits(out[2]), bits(y[2])), f"neighbours of a row with params {g}"
            assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[2]).all())


# ------------------------------------------------------------------------------------------ 4. adjoint identity
@pytest.mark.parametrize("fi", range(len(Y.FLUTTERS)))
@pytest.mark.parametrize("n", [33, 257, 4099, 16000])
def test_adjoint_identity(awm, dev, n, fi):
    u, params = Y.case(n, fi)
    v = np.random.default_rng(3000 * n + fi).standard_normal(u.shape).astype(np.float32)
    Wu = launch(dev, u, params).astype(np.float64)
    Wtv = launch(dev, v, params, adjoint=True).astype(np.float64)
    lhs, rhs = (Wu * v).sum(axis=1), (u * Wtv).sum(axis=1)
    room = (np.abs(v) * Y.case_ref(n, fi, False)[1]).sum(axis=1) + (np.abs(u) * Y.adjoint(v, params, Y.table())[1]).sum(axis=1)
    live = room > 0
    print(f"n {n} flutter {Y.FLUTTERS[fi]}: |<Wu, v> - <u, W^T v>| / room {(np.abs(lhs - rhs)[live] / room[live]).max():.4f}")
    assert (np.abs(lhs - rhs) <= room).all() and live.sum() >= 10


# ------------------------------------------------------------------------------------------ 5. the tape node
def test_backward_is_the_adjoint_launch(awm, dev):
    from awm_amd import ops
    n = 257
    x64, p64 = Y.case(n, 2)
    rows = [1, 7, 12, 16, 22]
    x, params, tab = to_dev(x64[rows], dev).requires_grad_(True), to_dev(p64[rows], dev).requires_grad_(True), to_dev(Y.table(), dev)
    g = to_dev(np.random.default_rng(55).standard_normal((len(rows), n)), dev)
    y = ops.TimeWarpFn.apply(x, params, tab, Y.ZEROS, Y.RES)
    y.backward(g)
    assert params.grad is None, "the parameters are constants of the graph"
    assert torch.equal(bits(x.grad), bits(ops.time_warp(g, params.detach(), tab, adjoint=True))), "backward is the adjoint launch, bit for bit"
    assert torch.equal(bits(y.detach()), bits(ops.time_warp(x.detach(), params.detach(), tab)))
    gx, g64 = x.grad.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    _, bnd = Y.adjoint(g64, p64[rows], Y.table())
    for i, r in enumerate(rows):
        M = Y.matrix(p64[r], n, Y.table())
        err = np.abs(gx[i] - M.T @ g64[i])
        print(f"row {r}: gradient against the dense matrix, worst err / bound {(err / np.maximum(bnd[i], 1e-300)).max():.4f}")
        assert (err <= bnd[i] + 1e-12 * np.abs(M.T).dot(np.abs(g64[i]))).all()
        assert np.abs(M).sum() > 10


# ------------------------------------------------------------------------------------------ 6. the module
@pytest.mark.parametrize("shape", [(5, 1, 2500), (2, 1300), (700,)])
def test_module_is_the_launch_with_its_draws(awm, dev, shape):
    from awm_amd import attacks, ops
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    x = to_dev(np.random.default_rng(61).standard_normal(shape), dev)
    kw = dict(speed=(0.8, 1.25), shift_s=(-0.002, 0.002), flutter_hz=(0.5, 8.0), flutter_depth=(0.0, 0.25), seed=8)
    att = awm.TimeWarp(**kw)
    y = att(x, row0=4)
    assert y.shape == x.shape and y.is_cuda and att.draw == 1 and not att.last_params.is_cuda
    want = Y.warp_params(8, 0, 4 + np.arange(rows), kw["speed"], kw["shift_s"], kw["flutter_hz"], kw["flutter_depth"])
    assert np.array_equal(att.last_params.numpy(), want), "the draws are the yardstick's"
    assert np.array_equal(attacks.row_warp_params(8, 0, 4 + np.arange(rows), kw["speed"], kw["shift_s"], kw["flutter_hz"], kw["flutter_depth"], 16000), want)
    assert torch.equal(bits(y.reshape(rows, -1)), bits(ops.time_warp(x.reshape(rows, -1), to_dev(want, dev))))
    ref, bnd = Y.forward(x.cpu().numpy().reshape(rows, -1), want, Y.table())
    assert (np.abs(y.cpu().numpy().reshape(rows, -1) - ref) <= bnd).all()
    b = att(x, row0=4)
    assert att.draw == 2 and not torch.equal(b, y)
    assert torch.equal(bits(att.reset()(x, row0=4)), bits(y)) and torch.equal(bits(att.reset(1)(x, row0=4)), bits(b)), "reset rewinds"
    if rows > 2:
        whole = att.reset()(x)
        parts = torch.cat([att.reset()(x[:2]), att.reset()(x[2:], row0=2)])
        assert torch.equal(bits(whole), bits(parts)), "a batch cut into pieces draws what the whole batch does"
    cpu = awm.TimeWarp(**kw)(x.cpu(), row0=4)
    assert (np.abs(cpu.numpy().reshape(rows, -1) - ref) <= bnd).all(), "and the CPU path is within the same bound of float64"


# ------------------------------------------------------------------------------------------ 7. refusals
def test_bad_arguments(awm, dev):
    from awm_amd import ops
    for args in Y.BAD_ARGS:
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm.lib.wm_time_warp(*args)
    x, p, tab = torch.zeros(3, 100, device=dev), torch.zeros(3, 6, device=dev), to_dev(Y.table(), dev)
    for bx, bp, bt in ((x, torch.zeros(2, 6, device=dev), tab), (x, torch.zeros(3, 5, device=dev), tab), (x, torch.zeros(18, device=dev), tab),
                       (x, p.double(), tab), (x.double(), p, tab), (x, p, tab[:-1]), (x, p, tab.double()), (x, p, tab.view(2, -1)),
                       (torch.zeros(3, 0, device=dev), p, tab), (torch.zeros(0, 100, device=dev), torch.zeros(0, 6, device=dev), tab),
                       (torch.zeros((), device=dev), p[:1], tab)):
        with pytest.raises(ValueError):
            ops.time_warp(bx, bp, bt)
    for kw in (dict(zeros=3), dict(zeros=33), dict(res=500), dict(res=32), dict(zeros=32, res=1024), dict(zeros=8), dict(res=256)):
        with pytest.raises(ValueError):
            ops.time_warp(x, p, tab, **kw)
    with pytest.raises(RuntimeError):
        ops.time_warp(x.cpu(), p, tab)
    with pytest.raises(RuntimeError):
        ops.time_warp(x, p.cpu(), tab)
    with pytest.raises(RuntimeError):
        ops.time_warp(x, p, tab.cpu())
    with pytest.raises(TypeError):
        ops.time_warp(x, [0.0] * 6, tab)
    torch.cuda.synchronize()


@pytest.mark.parametrize("zeros,res", [(4, 64), (8, 1024), (32, 512)])
def test_other_table_sizes(awm, dev, zeros, res):
    """the smallest table, a fine one, and one above 64 KiB of LDS"""
    from awm_amd import ops
    n = 1025
    x, params = Y.case(n, 1)
    pick = [5, 11, 21]
    tab = Y.table(zeros, res)
    for adj in (False, True):
        ref, bnd = (Y.adjoint if adj else Y.forward)(x[pick], params[pick], tab, zeros, res)
        y = ops.time_warp(to_dev(x[pick], dev), to_dev(params[pick], dev), to_dev(tab, dev), adjoint=adj, zeros=zeros, res=res).cpu().numpy()
        err = np.abs(y - ref)
        print(f"zeros {zeros} res {res} adjoint {adj}: worst err / bound {(err / np.maximum(bnd, 1e-300)).max():.4f}")
        assert (err <= bnd).all() and np.abs(ref).max() > 0.1


# ------------------------------------------------------------------------------------------ 8., 9. the training step and the robustness loop
def test_train_step_through_the_warp(awm, dev):
    """T = 2048: the shortest clip the step's loudness loss accepts"""
    G, D = reference_models(awm, dev)
    s = O.synthetic_clips(2, seed=41, T=2048).to(dev)
    msg = torch.tensor([3, 60001], device=dev)
    codec = torch.nn.Sequential(awm.TimeWarp(speed=(0.9, 1.1), flutter_hz=4.0, flutter_depth=0.01, seed=3), awm.PcmCodec(grad="straight_through"))
    G.train(); D.train()
    opt = torch.optim.Adam(list(G.parameters()) + list(D.parameters()), lr=1e-3)
    out = awm.train_step(G, D, opt, s, msg, codec=codec)
    assert codec[0].draw == 1 and tuple(codec[0].last_params.shape) == (2, 6)
    for k, v in out.items():
        if torch.is_tensor(v) and v.dim() == 0:
            assert bool(torch.isfinite(v)), f"loss {k}"
    assert bool(torch.isfinite(out["total"]))
    for k, p in G.named_parameters():
        assert bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), f"Generator {k}"


def test_evaluate_robustness_with_the_warp(awm, dev):
    ck = np.load(os.path.join(os.path.dirname(__file__), "golden", "detector_best_unprefixed.npz"))
    D = awm.Detector(16)
    D.load_state_dict({k: torch.from_numpy(ck[k]) for k in ck.files})
    torch.manual_seed(17)
    G = awm.Generator(16)
    G.to(dev); D.to(dev)
    batches = [O.synthetic_clips(2, seed=51, T=2048), O.synthetic_clips(2, seed=52, T=2048)]
    messages = [torch.tensor([3, 60001]), torch.tensor([77, 12345])]
    atk = {"speed_1.05": awm.TimeWarp(speed=1.05), "speed_1": awm.TimeWarp(speed=1.0)}
    res = awm.evaluate_robustness(G, D, batches, atk, device=dev, messages=messages)
    print(res)
    assert list(res) == ["none", "speed_1.05", "speed_1"]
    keys = ["bit_accuracy", "clean_prob", "delta_rms", "watermarked_prob"]
    assert sorted(res["speed_1.05"]) == keys and all(np.isfinite(res["speed_1.05"][k]) for k in keys)
    assert atk["speed_1.05"].draw == 2, "one call per batch, on the concatenation of s + delta and s"
    for k in keys:
        assert res["speed_1"][k] == res["none"][k], "speed 1 without a shift is the identity"
