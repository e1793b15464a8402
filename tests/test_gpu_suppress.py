"""wm_noise_suppress, awm_amd.noise_suppress / NoiseSuppress and their wiring on the GPU against the float64 yardstick of
tests/suppress_yardstick.py (numpy from the definition in include/wm_hip.h; nothing from the package).  Inputs sit one float into their
buffers, at a pointer = 4 (mod 8).

Bars (none tuned to the kernel):
  floats     relative L2 per row for y, max-abs for G and for N / max N, each at 8 x the error of the yardstick's own float32 twin against
             its float64 mode on the launch's own rows (the largest over those rows).  The 8 is the factor test_gpu_masking.py uses: it
             covers a radix-2 butterfly and reductions that order sums differently from a matrix product, and the device's log / exp.
             Where a row's twin error is exactly 0 the device's error on that row must be exactly 0 too.
  bits       reduce_db of 0 / NaN / 75 against the clipped values, two launches, a row alone / first of three / last of five, autograd
             against the direct call, the module against the functional, evaluate_robustness against direct calls: identical bits.
Every reference is computed once (lru_cache in the yardstick) and never written to.

Measured on an MI355X (floors, errors and err / bar per case, printed by every case): see DESIGN.md section 4v."""
import copy
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import wm_oracle as O

import suppress_yardstick as Y
from gpu_support import awm, dev  # noqa: F401
from gpu_support import bits, reference_models

pytestmark = pytest.mark.gpu


def S():
    return importlib.import_module("awm_amd.suppress")


def off_by_one_float(a, dev):
    """the same values in a buffer that starts 4 bytes earlier: the returned tensor's pointer is 4 (mod 8)"""
    a = np.array(a, dtype=np.float32, order="C")                  # a copy: the yardstick's cases are read-only
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
    buf[1:] = torch.from_numpy(a.reshape(-1)).to(dev)
    t = buf[1:].view(a.shape)
    assert t.data_ptr() % 8 == 4
    return t


def raw(awm, xd, rd, src=None, noise=None, alpha=Y.ALPHA, over=Y.OVER):
    """the C call on contiguous device rows: (y, G (rows, M, 257), N (rows, 257)); y is prefilled: every sample must be written"""
    rows, n = xd.shape
    frames, need = S().suppress_plan(rows, n)
    dev = xd.device
    y = torch.full((rows, n), 7.0, device=dev)
    G, N = torch.full((rows, frames, 257), 7.0, device=dev), torch.full((rows, 257), 7.0, device=dev)
    scratch = torch.empty(need // 4, dtype=torch.int32, device=dev)
    rd = torch.as_tensor(rd, dtype=torch.float32).to(dev)
    awm.lib.wm_noise_suppress(xd.data_ptr(), None if src is None else src.data_ptr(), None if noise is None else noise.data_ptr(), rd.data_ptr(),
                              y.data_ptr(), G.data_ptr(), N.data_ptr(), scratch.data_ptr(), rows, n, alpha, over,
                              torch.cuda.current_stream().cuda_stream)
    assert not bool((y == 7.0).any()) and not bool((G == 7.0).any()) and not bool((N == 7.0).any()), "every output is written"
    return y, G, N


def compare(label, got, r64, r32):
    """the launch's (y, G, N) against the float64 rows, at 8 x the twin's largest error over the launch's rows"""
    y, G, N = (t.cpu().numpy() for t in got)
    floors = [Y.errors(b, a) for a, b in zip(r64, r32)]
    errs = [Y.errors((y[i], G[i], N[i]), r64[i]) for i in range(len(r64))]
    top = [max(f[j] for f in floors) for j in range(3)]
    worst = [max(e[j] for e in errs) for j in range(3)]
    print(f"{label}: floors y {top[0]:.2e} G {top[1]:.2e} N {top[2]:.2e} | errors y {worst[0]:.2e} G {worst[1]:.2e} N {worst[2]:.2e} | "
          f"err / bar {worst[0] / (8 * top[0] + 1e-300):.3f} {worst[1] / (8 * top[1] + 1e-300):.3f} {worst[2] / (8 * top[2] + 1e-300):.3f}")
    for i, (f, e) in enumerate(zip(floors, errs)):
        for j, what in enumerate(("y", "G", "N")):
            if f[j] == 0.0:
                assert e[j] == 0.0, (label, i, what, "the twin is exact here: so must the device be")
            assert e[j] <= 8 * top[j], (label, i, what, e[j], top[j])


def chunk_frames():
    """the frames one workgroup of the analysis handles, read off the plan: the first frame count at which the scratch holds two chunks"""
    for M in range(2, 4096):
        need = S().suppress_plan(1, (M - 1) * 256)[1]
        if (need - M * 257 * 4) // (257 * 8 + 4) == 2:
            return M - 1
    raise AssertionError("the plan never reports a second chunk")


def size(label):
    c = chunk_frames()
    return {"seam": (c - 1) * 256, "seam+hop": c * 256, "two chunks+1": (2 * c - 1) * 256 + 1}.get(label, label)


# ------------------------------------------------------------------------------------------ 1. shapes and accuracy
@pytest.mark.parametrize("label", [1, 255, 256, 257, 511, 512, 513, 768, 1280, 16000, "seam", "seam+hop", "two chunks+1"])
def test_three_rows_against_float64(awm, dev, label):
    n = size(label)
    if isinstance(label, str):
        c = chunk_frames()
        assert Y.frame_count(n) == {"seam": c, "seam+hop": c + 1, "two chunks+1": 2 * c + 1}[label]
    xd = off_by_one_float(Y.case(n), dev)
    got = raw(awm, xd, Y.REDUCE_DB)
    compare(f"n {n} forward", got, Y.ref(n), Y.ref(n, twin=True))
    dy = off_by_one_float(Y.cotangent(n), dev)
    back = raw(awm, xd, Y.REDUCE_DB, src=dy)
    assert torch.equal(bits(back[1]), bits(got[1])) and torch.equal(bits(back[2]), bits(got[2])), "the gains come from x alone"
    compare(f"n {n} backward", back, Y.ref(n, "backward"), Y.ref(n, "backward", True))
    prof = off_by_one_float(Y.profile(n), dev)
    given = raw(awm, xd, Y.REDUCE_DB, noise=prof)
    assert torch.equal(bits(given[2]), bits(prof)), "a given profile is N"
    compare(f"n {n} profile", given, Y.ref(n, "profile"), Y.ref(n, "profile", True))
    y = awm.noise_suppress(xd, torch.tensor(Y.REDUCE_DB))
    assert torch.equal(bits(y), bits(got[0]))


def test_one_long_row_from_offset_pointers(awm, dev):
    n = 16000 * 4 + 13
    xd = off_by_one_float(Y.case(n)[0:1], dev)
    got = raw(awm, xd, Y.REDUCE_DB[0:1])
    assert got[1].shape[1] == Y.frame_count(n) == 252
    compare(f"n {n} one row", got, Y.ref(n)[0:1], Y.ref(n, twin=True)[0:1])
    back = raw(awm, xd, Y.REDUCE_DB[0:1], src=off_by_one_float(Y.cotangent(n)[0:1], dev))
    compare(f"n {n} one row backward", back, Y.ref(n, "backward")[0:1], Y.ref(n, "backward", True)[0:1])


# ------------------------------------------------------------------------------------------ 2. bits
def test_reduce_db_is_clipped_and_launches_are_reproducible(awm, dev):
    n = size("two chunks+1")
    xd = off_by_one_float(Y.case(n), dev)
    odd = raw(awm, xd, [float("nan"), 75.0, 0.0])
    want = raw(awm, xd, [0.0, 60.0, 0.0])
    again = raw(awm, xd, [0.0, 60.0, 0.0])
    for a, b, c in zip(odd, want, again):
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(b), bits(c))
    assert bool((want[1][0] == 1.0).all()) and bool((want[1][2] == 1.0).all()), "reduce_db = 0: every gain is exactly 1"
    assert float(want[1][1].min()) == float(np.float32(1e-3)) and float((want[0][0] - xd[0]).abs().max()) < 1e-6
    r60 = Y.model(Y.case(n)[1], 60.0)
    assert Y.errors((want[0][1].cpu().numpy(), want[1][1].cpu().numpy(), want[2][1].cpu().numpy()), r60)[0] < 1e-5


def test_rows_are_independent(awm, dev):
    n = size("two chunks+1")
    xd = off_by_one_float(Y.case(n), dev)
    dy = off_by_one_float(Y.cotangent(n), dev)
    rd = torch.tensor(Y.REDUCE_DB)
    one = raw(awm, xd, rd, src=dy)
    other = off_by_one_float(np.pad(Y.case(size("seam"))[:2], ((0, 0), (0, n - size("seam")))), dev)
    alone = raw(awm, xd[1:2].clone(), rd[1:2], src=dy[1:2].clone())
    first = raw(awm, xd[[1, 0, 2]], rd[[1, 0, 2]], src=dy[[1, 0, 2]])
    last = raw(awm, torch.cat([other, xd[[2, 0, 1]]]), torch.tensor([6.0, 30.0, 24.0, 12.0, 18.0]), src=torch.cat([other, dy[[2, 0, 1]]]))
    for got, r in ((alone, 0), (first, 0), (last, 4)):
        assert all(torch.equal(bits(a[r]), bits(b[1])) for a, b in zip(got, one)), "a row's bits know nothing of the batch"


def test_autograd_and_module_are_the_direct_call(awm, dev):
    n = 1280
    xd = off_by_one_float(Y.case(n), dev)
    dy = off_by_one_float(Y.cotangent(n), dev)
    m = awm.NoiseSuppress((6, 24), seed=9).to(dev)
    xl = xd[:, None].clone().requires_grad_(True)
    y = m(xl)
    y.backward(dy[:, None])
    rd = m.last_reduce_db
    assert np.array_equal(rd.numpy(), awm.attacks.row_reduce_db(9, 0, np.arange(3), (6, 24))) and m.draw == 1
    fwd, bwd = raw(awm, xd, rd), raw(awm, xd, rd, src=dy)
    assert tuple(y.shape) == (3, 1, n) and torch.equal(bits(y.detach()[:, 0]), bits(fwd[0]))
    assert tuple(xl.grad.shape) == (3, 1, n) and torch.equal(bits(xl.grad[:, 0]), bits(bwd[0])), "the backward is the same launch on dy"
    assert torch.equal(bits(awm.noise_suppress(xd, rd)), bits(fwd[0])), "the module is the functional at its draws"
    yg, G, N = awm.noise_suppress(xd[:, None], rd, gains_out=True)
    assert tuple(yg.shape) == (3, 1, n) and torch.equal(bits(G), bits(fwd[1])) and torch.equal(bits(N), bits(fwd[2]))
    assert tuple(awm.noise_suppress(xd[2], 18.0).shape) == (n,)
    host = awm.noise_suppress(xd.cpu(), rd)
    assert float((host - fwd[0].cpu()).norm() / host.norm()) < 1e-5, "the host path is the float64 restatement"
    prof = torch.from_numpy(np.array(Y.profile(n)))
    mp = awm.NoiseSuppress(18, noise_psd=prof).to(dev)
    assert mp.noise_psd.is_cuda and torch.equal(bits(mp(xd)), bits(raw(awm, xd, [18.0] * 3, noise=prof.to(dev))[0]))


# ------------------------------------------------------------------------------------------ 3. edge rows
def test_edge_rows(awm, dev):
    n = 1280
    x = Y.case(n)
    xs = np.stack([x[0], np.zeros(n, dtype=np.float32), x[2]])
    y, G, N = raw(awm, off_by_one_float(xs, dev), [18.0] * 3)
    assert not y[1].any() and bool(torch.isfinite(G[1]).all()) and bool(torch.isfinite(N[1]).all()), "silence in, exact zeros out"
    clean = raw(awm, off_by_one_float(x, dev), [18.0] * 3)
    for pos in (0, 700, n - 1):
        xb = np.array(x)
        xb[1, pos] = np.nan
        bad = raw(awm, off_by_one_float(xb, dev), [18.0] * 3)
        assert all(bool(torch.isnan(t[1]).all()) for t in bad), pos
        for i in (0, 2):
            assert all(torch.equal(bits(a[i]), bits(b[i])) for a, b in zip(bad, clean)), (pos, i)
    xb = np.array(x)
    xb[1, 5] = np.inf
    assert all(bool(torch.isnan(t[1]).all()) for t in raw(awm, off_by_one_float(xb, dev), [18.0] * 3))


# ------------------------------------------------------------------------------------------ 4. wiring
def test_evaluate_robustness_with_the_denoiser(awm, dev):
    from awm_amd.step import _eval_reductions
    G, D = reference_models(awm, dev)
    B, T = 3, 16000
    batches = [O.synthetic_clips(B, seed=71, T=T)]
    messages = [torch.tensor([3, 60001, 77])]
    res = awm.evaluate_robustness(G, D, batches, {"denoise": awm.NoiseSuppress(18)}, device=dev, messages=messages, quality=("stoi", "nmr"))
    print(res)
    assert list(res) == ["none", "denoise"]
    assert all(math.isfinite(v) for v in res["denoise"].values()), res["denoise"]
    s = batches[0].to(dev)
    with torch.no_grad():
        delta = awm.postprocess(G(s, messages[0].to(dev)))
        both, ref2 = torch.cat([s + delta, s], dim=0), torch.cat([s, s], dim=0)
        attacked = awm.NoiseSuppress(18)(both)
        assert torch.equal(bits(attacked), bits(awm.noise_suppress(both, 18.0)))
        out = _eval_reductions(D(attacked), messages[0].to(dev), delta)
    m = awm.masking(ref2, attacked)
    d, _ = awm.dsp.stoi(ref2, attacked)
    assert res["denoise"]["nmr_db"] == float(m.nmr_db[:B].cpu().double().mean()), "bit for bit a direct call on the same tensors"
    assert res["denoise"]["nmr_db_attack_only"] == float(m.nmr_db[B:].cpu().double().mean())      # the NMR columns are pooled on the host
    assert res["denoise"]["stoi_rows"] == B and res["denoise"]["stoi"] == float(d[:B].double().mean())
    assert res["denoise"]["watermarked_prob"] == float(out["prob_watermarked"].double().mean())
    assert res["denoise"]["nmr_db_attack_only"] > -math.inf, "the suppressor changes the clean half too"


def test_train_step_against_the_denoiser(awm, dev):
    G0, D0 = (m.train() for m in reference_models(awm, dev))
    s = O.synthetic_clips(2, seed=41, T=2048).to(dev)
    msg = torch.tensor([3, 60001], device=dev)
    G, D = copy.deepcopy(G0), copy.deepcopy(D0)
    opt = torch.optim.Adam(list(G.parameters()) + list(D.parameters()), lr=1e-3)
    codec = awm.NoiseSuppress((6, 24))
    out = awm.train_step(G, D, opt, s, msg, codec=codec)
    assert codec.draw >= 1 and codec.last_reduce_db is not None
    assert all(math.isfinite(float(v.detach())) for k, v in out.items() if isinstance(v, torch.Tensor) and v.numel() == 1), out
    grads = [p.grad for p in G.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and any(bool(g.any()) for g in grads)
    print(f"train step behind NoiseSuppress: total {float(out['total'].detach()):.5f}, reduce_db {codec.last_reduce_db.tolist()}")


# ------------------------------------------------------------------------------------------ 5. refusals
def test_bad_arguments(awm, dev):
    st = torch.cuda.current_stream().cuda_stream
    rows, n = 3, 2000
    frames, need = S().suppress_plan(rows, n)
    x, src = torch.zeros(rows, n, device=dev), torch.zeros(rows, n, device=dev)
    noise, rd = torch.ones(rows, 257, device=dev), torch.full((rows,), 12.0, device=dev)
    y, G, N = torch.full((rows, n), 7.0, device=dev), torch.full((rows, frames, 257), 7.0, device=dev), torch.full((rows, 257), 7.0, device=dev)
    sc = torch.zeros(need // 4, dtype=torch.int32, device=dev)
    px, pd, pn, pr, py, pg, po, ps = (t.data_ptr() for t in (x, src, noise, rd, y, G, N, sc))
    ok = (px, pd, pn, pr, py, pg, po, ps, rows, n, 0.98, 1.0, st)
    nan, inf = float("nan"), float("inf")
    for i, v in ((8, 0), (9, 0), (9, 2 ** 34 + 1), (8, 2 ** 40), (0, None), (3, None), (4, None), (7, None),
                 (0, px + 2), (1, pd + 1), (2, pn + 2), (3, pr + 2), (4, py + 1), (5, pg + 2), (6, po + 2), (7, ps + 2),
                 (10, 1.0), (10, -0.1), (10, nan), (11, 0.0), (11, inf), (11, nan), (11, -1.0),
                 (4, px), (4, pd), (4, pr), (5, px), (5, py), (6, pn), (6, py), (7, px), (7, py), (7, pg)):
        args = list(ok)
        args[i] = v
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm.lib.wm_noise_suppress(*args)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((G == 7.0).all()) and bool((N == 7.0).all()) and not sc.any(), "a refused call writes nothing"
    awm.lib.wm_noise_suppress(*ok)
    awm.lib.wm_noise_suppress(px, px, None, pr, py, None, None, ps, rows, n, 0.0, 2.5, st)      # src == x, no profile, no extra outputs
    awm.lib.wm_noise_suppress(px, None, None, pr, py, None, None, ps, rows, n, 0.98, 1.0, st)
    torch.cuda.synchronize()
    assert not y.any() and bool((N == 1.0).all())
    with pytest.raises(ValueError):
        awm.noise_suppress(x, 12.0, src=src.cpu())
    with pytest.raises(ValueError):
        awm.noise_suppress(x, torch.zeros(2, device=dev))
