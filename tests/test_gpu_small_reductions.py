"""The small reductions behind the stem, embedding, LSTM and loss kernels (stem_reduce_kernel, embed_scatter_add_kernel,
lstm_wgrad_reduce_kernel, sum_scale2_kernel), which spread their part lists over whole workgroups, the stem's ds phase, and the head
backward with the loss gradient formed on load at more tiles than workgroups -- at the part counts at which the grouping changes: one part, fewer parts than
part-groups, a ragged last group, more parts than one pass of the unrolled loops takes, and a grid capped at two workgroups per CU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_support import awm, dev  # noqa: F401
from gpu_support import p, rel_err, rnd, st
from test_gpu_parity import FWD_TOL, check
from test_gpu_tail_in_head import FP32_ULP, bits_equal, fp64_losses, frames, head_params, messages

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------- stem
# (B, T) -> workgroups = slabs for stem_reduce_kernel: 1; 6 (3 clips x 2 tiles, the second 64 of 256 steps); 320; 560 tiles on a grid
# capped at 2 x 256 workgroups, so the first 48 workgroups take two tiles
STEM_SHAPES = [(1, 64), (3, 320), (40, 2048), (70, 2048)]
_stem_ref = {}


def stem_case(B, T):
    """inputs and the fp64 gradients of F.conv1d(s, w, b, padding=3) for the output gradient g; computed once per shape"""
    if (B, T) not in _stem_ref:
        s, w, g = rnd(B, 1, T, seed=71), rnd(64, 1, 7, seed=72, scale=0.3), rnd(B, 64, T, seed=73)
        sr, wr, br = s.double().requires_grad_(), w.double().requires_grad_(), torch.zeros(64, dtype=torch.float64, requires_grad=True)
        F.conv1d(sr, wr, br, padding=3).backward(g.double())
        _stem_ref[(B, T)] = (s, w, g, sr.grad, wr.grad, br.grad)
    return _stem_ref[(B, T)]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("ds_mode", ["null", "all", "half"])
@pytest.mark.parametrize("B,T", STEM_SHAPES)
def test_stem_bwd(awm, dev, B, T, ds_mode, accumulate):
    lib = awm.lib
    s, w, g, ds_ref, dw_ref, db_ref = stem_case(B, T)
    sd, wd, gd = s.to(dev), w.to(dev), g.to(dev)
    nds = {"null": 0, "all": B, "half": B // 2}[ds_mode]
    dw0, db0 = rnd(64, 1, 7, seed=74), rnd(64, seed=75)           # what accumulate = 1 adds to
    res = []
    for _ in range(2):
        ds = None if ds_mode == "null" else torch.full((B, 1, T), 7.0, device=dev)
        dw, db = dw0.to(dev), db0.to(dev)
        part = torch.full((512 * 512,), float("nan"), device=dev)
        lib.wm_stem_bwd(p(gd), p(sd), p(wd), p(ds), p(part), p(dw), p(db), B, T, nds, accumulate, st())
        res.append((ds, dw, db))
    (ds, dw, db), (ds2, dw2, db2) = res
    assert bits_equal(dw, dw2) and bits_equal(db, db2), "two launches differ"
    base_w, base_b = (dw0.double(), db0.double()) if accumulate else (0.0, 0.0)
    check(dw.cpu(), (dw_ref + base_w).float(), FWD_TOL, "stem dw")
    check(db.cpu(), (db_ref + base_b).float(), FWD_TOL, "stem db")
    if ds is not None:
        assert bits_equal(ds, ds2), "two launches differ: ds"
        if nds:
            check(ds[:nds].cpu(), ds_ref[:nds].float(), FWD_TOL, "stem ds")
        assert bool((ds[nds:] == 7.0).all()), "ds rows >= nds must stay untouched"


# ------------------------------------------------------------------------------- embedding gradient
NROWS = 65536


def _ids(kind):
    g = torch.Generator().manual_seed(81)
    if kind == "one":
        return torch.tensor([4242], dtype=torch.int64)
    if kind == "all_equal":
        return torch.full((256,), 60001, dtype=torch.int64)
    if kind == "four_rows":
        return torch.tensor([0, 77, 65535, 300], dtype=torch.int64)[torch.randint(0, 4, (256,), generator=g)]
    if kind == "random300":
        return torch.randint(0, NROWS, (300,), generator=g, dtype=torch.int64)
    if kind == "b5000":                                           # every id many times, spread over 79 id chunks
        return torch.randint(0, 50, (5000,), generator=g, dtype=torch.int64) * 1000
    if kind == "out_of_range":                                    # ids outside the table get no gradient and disturb nothing
        m = torch.randint(0, 6, (70,), generator=g, dtype=torch.int64)
        m[::5] = -1
        m[3::7] = NROWS
        m[64] = 1 << 40
        return m
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["one", "all_equal", "four_rows", "random300", "b5000", "out_of_range"])
def test_embed_scatter_add(awm, dev, kind):
    lib = awm.lib
    msg = _ids(kind)
    B = msg.numel()
    dvec = rnd(B, 64, seed=82)
    want = np.zeros((NROWS, 64), dtype=np.float32)
    dv = dvec.numpy()
    for b in range(B):                                            # the serial float32 walk over the batch
        m = int(msg[b])
        if 0 <= m < NROWS:
            want[m] = want[m] + dv[b]
    table, msg_d, dvec_d = torch.zeros(NROWS, 64, device=dev), msg.to(dev), dvec.to(dev)
    lib.wm_embed_scatter_add(p(table), p(msg_d), p(dvec_d), B, NROWS, st())
    assert bits_equal(table.cpu(), torch.from_numpy(want)), "not the batch-order float32 sum (or a row outside the ids was written)"


# ------------------------------------------------------------------------------- LSTM weight gradients
def _lstm_params():
    g = torch.Generator().manual_seed(90)
    k = 1.0 / 8.0
    wi, wh = (torch.rand(256, 64, generator=g) * 2 - 1) * k, (torch.rand(256, 64, generator=g) * 2 - 1) * k
    bi, bh = (torch.rand(256, generator=g) * 2 - 1) * k, (torch.rand(256, generator=g) * 2 - 1) * k
    return wi, wh, bi, bh


# B = slabs for lstm_wgrad_reduce_kernel (8 part-groups): 1, 3 and 5 leave groups empty; 40 gives every group five slabs (one pass
# of the four-accumulator loop and a one-slab tail)
@pytest.mark.parametrize("B,T", [(1, 64), (3, 96), (5, 64), (40, 64)])
def test_lstm_wgrad_reduce(awm, dev, B, T):
    from awm_amd import ops
    lib = awm.lib
    wi, wh, bi, bh = _lstm_params()
    x, gg = rnd(B, 64, T, seed=91), rnd(B, 64, T, seed=92)
    grads = []
    for ws in (True, False):
        xd, wid, whd, bid, bhd = (t.to(dev).requires_grad_() for t in (x, wi, wh, bi, bh))
        with ops.switches(lstm_bwd_ws=ws):
            ops.LSTMFn.apply(xd, wid, whd, bid, bhd).backward(gg.to(dev))
        grads.append([t.grad.clone() for t in (xd, wid, whd, bid, bhd)])
    assert torch.equal(grads[0][0], grads[1][0]), "dx differs from the two-launch path"
    for name, a, b_ in zip(("dW_ih", "dW_hh", "db_ih", "db_hh"), grads[0][1:], grads[1][1:]):
        assert rel_err(a, b_) < 2e-6, (name, rel_err(a, b_))
    # accumulate = 1 through the C ABI: a second call on the same activations adds the same sums to the first call's
    xd, dh = x.to(dev), gg.to(dev)
    wid, whd, bid, bhd = (t.to(dev) for t in (wi, wh, bi, bh))
    h, gates, cst = torch.empty_like(xd), torch.empty(B, T, 256, device=dev), torch.empty(B, T, 64, device=dev)
    lib.wm_lstm_fwd_fused(p(xd), p(wid), p(bid), p(bhd), p(whd), p(h), p(gates), p(cst), B, T, st())
    dst = [torch.full_like(t, float("nan")) for t in (wid, whd, bid, bhd)]
    first = None
    for acc in (0, 1):
        ga = gates.clone()                                        # the launch overwrites the saved activations with da
        part = torch.full((B * (256 * 128 + 256),), float("nan"), device=dev)
        lib.wm_lstm_bwd_wgrad(p(ga), p(cst), p(dh), p(whd), p(xd), p(h), p(part), *map(p, dst), B, T, acc, st())
        if acc == 0:
            first = [t.clone() for t in dst]
    for name, a, f, ref in zip(("dW_ih", "dW_hh", "db_ih", "db_hh"), dst, first, grads[1][1:]):
        assert rel_err(f, ref) < 2e-6, (name, rel_err(f, ref))
        assert bits_equal(a, f + f), f"{name}: accumulate = 1 did not add the same sums"


# ------------------------------------------------------------------------------- the two BCE sums
# (R, B, T) -> R * ceil(T / 256) partials per sum for sum_scale2_kernel: 1, 3 and 260
@pytest.mark.parametrize("R,B,T", [(1, 1, 64), (3, 1, 200), (130, 65, 512)])
def test_loss_sums(awm, dev, R, B, T):
    lib = awm.lib
    NO = 17
    x, y2, sc, sh = frames(R, T, dev)
    w, b = head_params(NO, dev)
    msg = messages(B, NO, "mixed", dev)
    nblk = R * ((T + 255) // 256)
    got = []
    for _ in range(2):
        lg = torch.empty(R, T, NO, device=dev)
        part = torch.full((2 * nblk,), float("nan"), device=dev)
        res = torch.full((2,), 123.0, device=dev)
        lib.wm_headN_tail_fwd(p(x), p(y2), p(sc), p(sh), p(w), p(b), p(msg), B, p(part), p(res[0]), p(res[1]), p(torch.empty_like(x)),
                              None, p(lg), R, T, NO, st())
        got.append((res.clone(), lg))
    assert bits_equal(got[0][0], got[1][0]) and bits_equal(got[0][1], got[1][1]), "two launches differ"
    res, lg = got[0]
    un = torch.full((2,), 123.0, device=dev)
    upart = torch.empty(2 * R * ((T * NO + 4095) // 4096), device=dev)
    lib.wm_bce_fwd(p(lg), p(msg), p(upart), p(un[0]), p(un[1]), B, R, T, NO, st())
    for k, ref in zip((0, 1), fp64_losses(lg, msg, B)):
        e_f, e_u = abs(float(res[k]) - ref), abs(float(un[k]) - ref)
        print(f"{('loc', 'bce')[k]} {ref:.9g}: head-forward sums err {e_f:.3e}, wm_bce_fwd err {e_u:.3e}")
        assert e_f <= 2.0 * e_u + FP32_ULP * abs(ref), f"{('loc', 'bce')[k]}: {e_f:.3e} vs wm_bce_fwd {e_u:.3e}"


def test_sum_scale_many_partials(awm, dev):
    """sum_scale2_kernel beyond one pass of its 1024 threads: wm_bce_fwd at 300 rows x 18 chunks = 5400 partials per sum (bench.py runs
    32 256) -- one pass of the four-accumulator loop, then 1304 / 280 / 0 elements in the three tails.  The kernel's contract is the fp64
    sum of the partials times the scale, rounded once to float: against torch's fp64 sum of the same partials (another order, so
    1e-13 apart before the rounding) the two floats are the same or neighbours."""
    lib = awm.lib
    R, B, T, NO = 300, 150, 4100, 17
    chunks = (T * NO + 4095) // 4096
    grid = chunks * R
    assert grid == 5400
    logits = rnd(R, T, NO, seed=101, scale=3.0).to(dev)
    msg = messages(B, NO, "mixed", dev)
    got = []
    for _ in range(2):
        part = torch.full((2 * grid,), float("nan"), device=dev)
        res = torch.full((2,), 123.0, device=dev)
        lib.wm_bce_fwd(p(logits), p(msg), p(part), p(res[0]), p(res[1]), B, R, T, NO, st())
        got.append((res.clone(), part))
    assert bits_equal(got[0][0], got[1][0]), "two launches differ"
    res, part = got[0]
    for k, scale in ((0, 1.0 / (R * T)), (1, 1.0 / (B * T * (NO - 1)))):
        ref = float(part[k * grid:(k + 1) * grid].double().sum()) * scale
        err = abs(float(res[k]) - ref)
        print(f"sum {k}: {ref:.9g} err {err:.3e}")
        assert err <= FP32_ULP * abs(ref), (k, float(res[k]), ref)
    loc64, bce64 = fp64_losses(logits, msg, B)
    assert abs(float(res[0]) - loc64) < 1e-5 * loc64 and abs(float(res[1]) - bce64) < 1e-5 * bce64      # the partials themselves are sane


# ------------------------------------------------------------------------------- head backward, loss gradient formed on load
# 5 rows x 63 tiles = 315 tiles on 256 workgroups: 59 of them prefetch and stage a second tile inside the main loop (the last of a
# clip is partial: 16000 = 62 * 256 + 128), which the shapes of tests/test_gpu_tail_in_head.py (at most 8 tiles) never do
@pytest.mark.parametrize("NO", [17, 33])
def test_headN_bwd_bce_second_tile(awm, dev, NO):
    lib = awm.lib
    R, B, T = 5, 2, 16000
    x = rnd(R, 64, T, seed=41).to(dev)
    w, _ = head_params(NO, dev)
    logits = rnd(R, T, NO, seed=42, scale=3.0).to(dev)
    msg = messages(B, NO, "mixed", dev)
    g_loc, g_bce = torch.tensor([10.0], device=dev), torch.tensor([1.0], device=dev)
    d = torch.empty_like(logits)
    lib.wm_bce_bwd(p(logits), p(msg), p(g_loc), p(g_bce), p(d), B, R, T, NO, st())
    for acc in (0, 1):
        res = []
        for fused in (False, True):
            dx = torch.full_like(x, float("nan"))
            dw, db = rnd(NO, 64, 1, seed=43).to(dev), rnd(NO, seed=44).to(dev)
            part = torch.full((256 * (NO * 64 + NO),), float("nan"), device=dev)
            if fused:
                lib.wm_headN_bwd_bce(p(logits), p(msg), p(g_loc), p(g_bce), p(x), p(w), p(dx), p(part), p(dw), p(db), B, R, T, NO, acc, st())
            else:
                lib.wm_headN_bwd(p(d), p(x), p(w), p(dx), p(part), p(dw), p(db), R, T, NO, acc, st())
            res.append((dx, dw, db))
        for a, c, nm in zip(res[0], res[1], ("dx", "dw", "db")):
            assert bits_equal(a, c), f"{nm} NO={NO} accumulate={acc}"
        assert bool(torch.isfinite(res[1][0]).all())
