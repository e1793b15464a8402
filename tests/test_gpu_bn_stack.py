"""csrc/bn.hip through its C ABI against the float64 yardsticks of tests/bn_yardstick.py: wm_bn_finalize, wm_bn_eval_scale_shift,
wm_bn_add_relu(_mask), wm_relu_bwd_reduce(_mask), wm_bn_bwd_finalize, wm_gscale_absmax, wm_gscale_from_max and wm_absmax_rows, each at
the shapes where it takes another path (the sixteen slices of the partial reduction, one mask dword, one unrolled iteration, the grid
cap) and on the inputs its formula has a branch for (a negative variance, count 1, no running statistics, eval mode, accumulate, a
maximum next to a power of two, all-zero / inf / NaN tensors).  Every bound is derived in bn_yardstick.py, and
tests/test_bn_yardstick_cpu.py shows a float32 restatement meeting it and a planted defect missing it.  Every output buffer has
CANARY untouched elements on either side.  Every comparison prints its error / bound; the worst per kernel stand in bn_yardstick.py."""
import numpy as np
import pytest
import torch

import bn_yardstick as Y
from gpu_support import CANARY, Guarded, awm, dev, invalid, p, st, to_dev  # noqa: F401
from yardstick_common import assert_within, ulp32

pytestmark = pytest.mark.gpu

assert CANARY == Y.CANARY            # the untouched elements on either side of every output (bn_yardstick.py, section C)


# --------------------------------------------------------------------------------------------------------------- 1. wm_bn_finalize
@pytest.mark.parametrize("name,nparts,per_part,running", Y.FIN_CASES)
def test_bn_finalize(awm, dev, name, nparts, per_part, running):
    inp = Y.finalize_inputs(nparts, per_part)
    ref = Y.finalize_ref(inp, running)
    part, gam, bet = (to_dev(inp[k], dev) for k in ("partials", "gamma", "beta"))
    rm, rv = Guarded(dev, 64, inp["running_mean"]), Guarded(dev, 64, inp["running_var"])
    nbt = Guarded(dev, 1, np.array([Y.NBT_START], dtype=np.int64), dtype=torch.int64)
    out = {k: Guarded(dev, 64) for k in ("scale", "shift", "save_mean", "save_invstd")}
    awm.lib.wm_bn_finalize(p(part), nparts, inp["count"], p(gam), p(bet), p(rm.t) if running else None, p(rv.t), p(nbt.t),
                           np.float32(0.1).item(), np.float32(1e-5).item(), *(p(out[k].t) for k in ("scale", "shift", "save_mean", "save_invstd")),
                           st())
    torch.cuda.synchronize()
    got = {k: g.np() for k, g in out.items()}
    got["running_mean"], got["running_var"] = rm.np(), rv.np()
    for k in Y.FIN_NAMES:
        assert np.all(np.isfinite(got[k])), f"{name} {k}: not finite"
        assert_within(got[k], ref[k], Y.finalize_bound(ref, k), f"wm_bn_finalize {name} {k}")
    for g in list(out.values()) + [rm, rv, nbt]:
        assert g.intact(), f"{name}: a canary next to an output changed"
    if per_part > 1:                              # the clamp: var < 0 -> invstd = 1 / sqrt(eps)
        assert abs(float(got["save_invstd"][Y.CH_CONST]) - 1.0 / np.sqrt(Y.EPS)) <= ulp32(1.0 / np.sqrt(Y.EPS))
        assert got["scale"][Y.CH_GAMMA0] == 0.0 and got["shift"][Y.CH_GAMMA0] == inp["beta"][Y.CH_GAMMA0]
    if running:
        assert int(nbt.t.item()) == Y.NBT_START + 1, "num_batches_tracked must advance by exactly one, as an int64"
    else:
        assert rm.intact(whole=True) and rv.intact(whole=True) and nbt.intact(whole=True), "running_mean == NULL: nothing of the running state moves"


# --------------------------------------------------------------------------------------------------------------- 2. producer chain
# A finding, kept as a strict expected failure: at |mean| / std = 30 the float32 one-pass sums of the convolution epilogues cost the
# variance of BN1 enough that the block's output and BN2's new running mean leave the bar -- measured 3.5 x and 2.3 x the bar at
# (1, 64), 1.6 x and 1.6 x at (3, 132) -- where the float32 oracle (two-pass statistics) stays at 0.1 of it.  At 0 and 3 everything is
# inside 0.07 of the bar.  The epilogues are not this file's to change.
OFF_CENTRE_30 = pytest.mark.xfail(strict=True, raises=AssertionError, reason="one-pass float32 sums in the convolution epilogues: at |mean| / std = 30 the ResBlock's "
                                  "output is 1.6 to 3.5 times the bar from float64 (the float32 oracle: 0.1)")
OFF_CENTRE_30_MISSES = ("out", "block.4.running_mean")
CHAIN_CASES = [pytest.param(r, B, T, marks=[OFF_CENTRE_30] if r == 30 else []) for r in Y.CHAIN_RATIOS for B, T in Y.CHAIN_SHAPES]


@pytest.mark.parametrize("ratio,B,T", CHAIN_CASES)
def test_producer_chain(awm, dev, ratio, B, T):
    """a whole ResBlock in training mode, BN1's input |mean| / std = ratio off-centre: the statistics of the convolution epilogues
    through wm_bn_finalize into everything behind them, against float64 (bn_yardstick.py, section G)"""
    sd, x, up = Y.chain_inputs(ratio, B, T)
    r64, r32 = Y.chain_ref(ratio, B, T)
    m = awm.ResBlock(64)
    m.load_state_dict(sd)
    m.to(dev).train()
    xd = x.to(dev).requires_grad_()
    out = m(xd)
    out.backward(up.to(dev))
    torch.cuda.synchronize()
    got = dict(out=out.detach(), dx=xd.grad)
    state, params = m.state_dict(), dict(m.named_parameters())
    for k in Y.CHAIN_NAMES[2:]:
        got[k] = state[k] if "running" in k else params[k].grad
    assert int(state["block.1.num_batches_tracked"]) == Y.CHAIN_NBT + 1 and int(state["block.4.num_batches_tracked"]) == Y.CHAIN_NBT + 1
    failed = {}
    for k in Y.CHAIN_NAMES:
        try:
            Y.held(got[k], r64[k], r32[k], Y.chain_floor(k, ratio), f"ResBlock ratio {ratio} ({B}, {T}) {k}")
        except AssertionError as e:
            failed[k] = str(e)
    # the expected failure covers the two tensors of the finding and nothing else: any other miss fails outright
    if ratio == 30 and not set(failed) <= set(OFF_CENTRE_30_MISSES):
        pytest.fail("at |mean| / std = 30 more than the known tensors miss the bar:\n" + "\n".join(failed.values()))
    assert not failed, "\n".join(failed.values())


# ------------------------------------------------------------------------------------------------------- 3. wm_bn_eval_scale_shift
def test_bn_eval_scale_shift(awm, dev):
    inp = Y.eval_inputs()
    ref = Y.eval_ref(inp)
    sc, sh = Guarded(dev, 64), Guarded(dev, 64)
    args = [to_dev(inp[k], dev) for k in ("gamma", "beta", "running_mean", "running_var")]
    awm.lib.wm_bn_eval_scale_shift(*map(p, args), np.float32(1e-5).item(), p(sc.t), p(sh.t), st())
    torch.cuda.synchronize()
    assert_within(sc.np(), ref["scale"], Y.eval_bound(ref, "scale"), "wm_bn_eval_scale_shift scale")
    assert_within(sh.np(), ref["shift"], Y.eval_bound(ref, "shift"), "wm_bn_eval_scale_shift shift")
    assert sc.intact() and sh.intact()


# --------------------------------------------------------------------------------------- 4. wm_bn_add_relu, wm_bn_add_relu_mask
@pytest.mark.parametrize("B", Y.TAIL_B)
@pytest.mark.parametrize("T", Y.TAIL_T)
def test_bn_add_relu_and_mask(awm, dev, B, T):
    x, y, sc, sh = Y.tail_inputs(B, T)
    ref, pos, bound = Y.tail_ref(x, y, sc, sh)
    want = Y.pack_mask(pos)
    xd, yd, scd, shd = (to_dev(a, dev) for a in (x, y, sc, sh))
    nw = (T + 31) // 32
    for masked in (False, True):
        out, mask = Guarded(dev, B * 64 * T), Guarded(dev, B * 64 * nw, dtype=torch.int32)
        if masked:
            awm.lib.wm_bn_add_relu_mask(p(xd), p(yd), p(scd), p(shd), p(out.t), p(mask.t), B, T, st())
        else:
            awm.lib.wm_bn_add_relu(p(xd), p(yd), p(scd), p(shd), p(out.t), B, T, st())
        torch.cuda.synchronize()
        got = out.np((B, 64, T))
        what = f"wm_bn_add_relu{'_mask' if masked else ''} ({B}, {T})"
        assert_within(got, ref, bound, what + " out")
        assert not got[~pos].any() and not np.signbit(got[~pos]).any(), what + ": +0.0 wherever the reference is not positive"
        assert out.intact() and mask.intact(whole=not masked), what + ": a canary changed"
        if masked:
            m = mask.np((B * 64, nw)).view(np.uint32)
            assert np.array_equal(m, want), what + ": the mask is not (reference > 0), bit t % 32 of dword t / 32, padding bits clear"


def test_bn_add_relu_invalid_arguments(awm, dev):
    B, T = 1, 32
    x, y, sc, sh = (to_dev(a, dev) for a in Y.tail_inputs(B, T))
    out, mask = Guarded(dev, B * 64 * T), Guarded(dev, B * 64, dtype=torch.int32)
    invalid(lambda: awm.lib.wm_bn_add_relu(p(x), p(y), p(sc), p(sh), p(out.t), B, 30, st()), out)
    invalid(lambda: awm.lib.wm_bn_add_relu_mask(p(x), p(y), p(sc), p(sh), p(out.t), p(mask.t), B, 30, st()), out, mask)
    invalid(lambda: awm.lib.wm_bn_add_relu_mask(p(x), p(y), p(sc), p(sh), p(out.t), None, B, T, st()), out, mask)


# ------------------------------------------------------------------------------- 5. wm_relu_bwd_reduce, wm_relu_bwd_reduce_mask
@pytest.mark.parametrize("B", Y.TAIL_B)
@pytest.mark.parametrize("T", Y.TAIL_T)
def test_relu_bwd_reduce(awm, dev, B, T):
    x, y, sc, sh = Y.tail_inputs(B, T)
    out64, pos, _ = Y.tail_ref(x, y, sc, sh)
    g = Y.reduce_inputs(B, T, pos)
    dz_ref, max_ref, part_ref, bound = Y.reduce_ref(g, y, pos)
    gd, yd, outd = to_dev(g, dev), to_dev(y, dev), to_dev(out64.astype(np.float32), dev)
    maskd = torch.from_numpy(Y.pack_mask(pos).view(np.int32)).to(dev)
    # (entry point, dz written, dzmax written)
    for masked, with_dz, with_max in ((False, True, False), (True, True, True), (True, True, False), (True, False, True), (True, False, False)):
        dz, part, dzmax = Guarded(dev, B * 64 * T), Guarded(dev, B * 128), Guarded(dev, B * 64)
        if masked:
            awm.lib.wm_relu_bwd_reduce_mask(p(gd), p(maskd), p(yd), p(dz.t) if with_dz else None, p(part.t), p(dzmax.t) if with_max else None,
                                            B, T, st())
        else:
            awm.lib.wm_relu_bwd_reduce(p(gd), p(outd), p(yd), p(dz.t), p(part.t), B, T, st())
        torch.cuda.synchronize()
        what = f"wm_relu_bwd_reduce{'_mask' if masked else ''} ({B}, {T}) dz={with_dz} dzmax={with_max}"
        assert_within(part.np((B, 2, 64)), part_ref, bound, what + " partial")
        assert part.intact() and dz.intact(whole=not with_dz) and dzmax.intact(whole=not with_max), what + ": a canary changed"
        if with_dz:
            assert np.array_equal(dz.np((B, 64, T)).view(np.int32), dz_ref.view(np.int32)), what + ": dz is g or +0.0 by the reference mask"
        if with_max:
            assert np.array_equal(dzmax.np().view(np.int32), max_ref.view(np.int32)), what + ": dzmax is the exact row maximum of |dz|"


def test_relu_bwd_reduce_invalid_arguments(awm, dev):
    B, T = 1, 32
    x, y, sc, sh = Y.tail_inputs(B, T)
    g, yd = to_dev(x, dev), to_dev(y, dev)
    mask = torch.zeros(B * 64, dtype=torch.int32, device=dev)
    dz, part, dzmax = Guarded(dev, B * 64 * T), Guarded(dev, B * 128), Guarded(dev, B * 64)
    invalid(lambda: awm.lib.wm_relu_bwd_reduce(p(g), p(g), p(yd), p(dz.t), p(part.t), B, 30, st()), dz, part)
    invalid(lambda: awm.lib.wm_relu_bwd_reduce_mask(p(g), p(mask), p(yd), p(dz.t), p(part.t), p(dzmax.t), B, 30, st()), dz, part, dzmax)
    invalid(lambda: awm.lib.wm_relu_bwd_reduce_mask(p(g), None, p(yd), p(dz.t), p(part.t), p(dzmax.t), B, T, st()), dz, part, dzmax)


# ---------------------------------------------------------------------------------------------------------- 6. wm_bn_bwd_finalize
def _bwd_finalize(awm, dev, inp, accumulate, eval_mode, dzmax=None, with_gs=False):
    """-> ({A, C, Bhi, Blo, dgamma, dbeta} numpy, gscale numpy or None); canaries checked"""
    part, gam, mu, inv = (to_dev(inp[k], dev) for k in ("partials", "gamma", "save_mean", "save_invstd"))
    A, Cc, Bc = Guarded(dev, 64), Guarded(dev, 64), Guarded(dev, 128)
    dg, db = Guarded(dev, 64, inp["dgamma0"]), Guarded(dev, 64, inp["dbeta0"])
    gs = Guarded(dev, 2)
    dzm = None if dzmax is None else to_dev(dzmax, dev)
    awm.lib.wm_bn_bwd_finalize(p(part), inp["partials"].shape[0], inp["count"], p(gam), p(mu), p(inv), p(A.t), p(Bc.t), p(Cc.t), p(dg.t), p(db.t),
                               accumulate, eval_mode, p(dzm), 0 if dzmax is None else dzmax.size, p(gs.t) if with_gs else None, st())
    torch.cuda.synchronize()
    for g in (A, Cc, Bc, dg, db):
        assert g.intact(), "a canary next to an output changed"
    assert gs.intact(whole=not with_gs)
    b = Bc.np()
    return dict(A=A.np(), C=Cc.np(), Bhi=b[:64], Blo=b[64:], dgamma=dg.np(), dbeta=db.np()), (gs.np() if with_gs else None)


@pytest.mark.parametrize("nparts,accumulate,eval_mode", Y.BWD_CASES)
def test_bn_bwd_finalize(awm, dev, nparts, accumulate, eval_mode):
    inp = Y.bwd_inputs(nparts)
    ref = Y.bwd_ref(inp, accumulate, eval_mode)
    got, _ = _bwd_finalize(awm, dev, inp, accumulate, eval_mode)
    what = f"wm_bn_bwd_finalize nparts={nparts} accumulate={accumulate} eval={eval_mode}"
    for k in ("A", "C", "dgamma", "dbeta"):
        assert_within(got[k], ref[k], Y.bwd_bound(ref, k, accumulate), f"{what} {k}")
    assert np.all(np.abs(got["Blo"].astype(np.float64)) <= ulp32(got["Bhi"]) / 2), what + ": Blo is no low word of Bhi"
    if eval_mode:
        for k in ("C", "Bhi", "Blo"):
            assert not got[k].view(np.int32).any(), f"{what}: {k} must be +0.0"
    else:
        res, mag = Y.zero_sum(inp, got["A"], got["C"], got["Bhi"], got["Blo"])
        print(f"{what}: zero-sum residue / (2^-45 of its terms) {np.max(res / (Y.ZERO_SUM * mag)):.3f}")
        assert np.all(res <= Y.ZERO_SUM * mag), what + ": A s1 + (Bhi + Blo) count + C mu count does not vanish"
        assert_within(got["Bhi"].astype(np.float64) + got["Blo"].astype(np.float64), ref["B"], 4 * ulp32(ref["B"]) + Y.TINY, f"{what} B")


@pytest.mark.parametrize("nmax", Y.BWD_NMAX)
def test_bn_bwd_finalize_gradient_scale(awm, dev, nmax):
    inp = Y.gscale_bwd_inputs()
    n = 0
    for m in Y.gs_maxima() + [np.float32(0.0), np.float32(np.inf)]:
        for where in ("first", "last"):
            got, gs = _bwd_finalize(awm, dev, inp, 0, 0, Y.dzmax_vector(m, nmax, where), with_gs=True)
            what = f"wm_bn_bwd_finalize gscale: max dzmax {m!r} ({where} of {nmax})"
            assert float(np.abs(got["A"]).max()) == 1.0
            if m == 0.0 or not np.isfinite(m):
                assert gs[0] == 1.0 and gs[1] == 1.0, what + ": scale 1 for an all-zero or infinite maximum"
                continue
            assert Y.is_pow2(gs[0]) and float(gs[0]) * float(gs[1]) == 1.0, what + f": gs {gs[0]!r} is no power of two"
            assert Y.in_interval(m, gs[0], 9), what + f": max |A| max |dz| gs = {float(m) * float(gs[0])!r} is outside (256, 512]"
            assert float(gs[0]) == Y.scale_exact(m, 9)
            n += 1
    assert n == 2 * len(Y.gs_maxima())
    A, Cc, Bc, dg, gsc = (Guarded(dev, k) for k in (64, 64, 128, 64, 2))
    part, v = to_dev(inp["partials"], dev), to_dev(inp["gamma"], dev)
    invalid(lambda: awm.lib.wm_bn_bwd_finalize(p(part), 16, inp["count"], p(v), p(v), p(v), p(A.t), p(Bc.t), p(Cc.t), p(dg.t), p(dg.t), 0, 0,
                                               None, 0, p(gsc.t), st()), A, Cc, Bc, dg, gsc)


# ------------------------------------------------------------------------ 7. wm_gscale_absmax, wm_gscale_from_max, wm_absmax_rows
def _scale_ok(m, L, gs, what):
    """the three properties of a scale for the maximum m (a float32), or {1, 1}"""
    m = np.float32(abs(m))
    if not (m > 0 and np.isfinite(m)):
        assert gs[0] == 1.0 and gs[1] == 1.0, what + f": {gs!r} for an all-zero, inf or NaN tensor, not {{1, 1}}"
        return
    assert Y.is_pow2(gs[0]), what + f": gs {gs[0]!r} is no power of two"
    assert float(gs[0]) * float(gs[1]) == 1.0, what + ": gscale[1] gscale[0] != 1"
    assert Y.in_interval(m, gs[0], L), what + f": max |x| gs = {float(m) * float(gs[0])!r} is outside (2^{L - 1}, 2^{L}]"
    assert float(gs[0]) == Y.scale_exact(m, L)


def _absmax(awm, x, L, scratch):
    gs = Guarded(x.device, 2)
    awm.lib.wm_gscale_absmax(p(x), x.numel(), p(scratch.t), float(L), p(gs.t), st())
    torch.cuda.synchronize()
    assert gs.intact() and scratch.intact()
    return gs.np()


@pytest.mark.parametrize("n", Y.GS_N)
def test_gscale_absmax(awm, dev, n):
    x = to_dev(Y.absmax_input(n, np.float32(1.0), "first"), dev)           # |x| < 1 / 2 but for the planted maximum
    scratch = Guarded(dev, 1024)
    places = ((0, 1.0), (n - 1, 1.0), (n - 1, -1.0))      # the first element, the last, negative; another one at the second target
    i = 0
    for L in Y.GS_L:
        for m in Y.gs_maxima():
            at, sign = places[i % 3]
            i += 1
            x.mul_(float(m) / float(x.abs().max()))                       # a power of two or close to it: the rest stays below m / 2
            x[0] = x[n - 1] = float(m) / 4
            x[at] = sign * float(m)
            assert float(x.abs().max()) == float(m)
            _scale_ok(m, L, _absmax(awm, x, L, scratch), f"wm_gscale_absmax n={n} m={sign * float(m)!r} at {at} L={L}")
    # among other data: fmaxf drops a NaN, so one NaN leaves the scale of the remaining maximum; one inf gives {1, 1}
    top = float(x.abs().max())
    x[n // 2] = float("nan")
    _scale_ok(np.float32(top), 12, _absmax(awm, x, 12, scratch), f"wm_gscale_absmax n={n}, one NaN among data with maximum {top!r}")
    x[n // 2] = float("-inf")
    _scale_ok(np.float32("inf"), 12, _absmax(awm, x, 12, scratch), f"wm_gscale_absmax n={n}, one -inf among data")
    for bad in (0.0, float("inf"), float("-inf"), float("nan")):
        x[n // 2] = bad
        if bad == 0.0:
            x.zero_()
        _scale_ok(np.float32(bad), 12, _absmax(awm, x, 12, scratch), f"wm_gscale_absmax n={n} with {bad}")
    x.fill_(float("nan"))
    _scale_ok(np.float32("nan"), 12, _absmax(awm, x, 12, scratch), f"wm_gscale_absmax n={n} all NaN")


def test_gscale_absmax_rearms_its_arrival_counter(awm, dev):
    """three launches in a row on one stream, with grids of 1, 1024 and 2 workgroups: the last workgroup of each must find the
    counter at zero"""
    xs = [to_dev(Y.absmax_input(n, np.float32(m), w, seed=n), dev) for n, m, w in ((4, 3.0, "first"), (Y.GS_N[-1], -700.0, "last"), (8196, 0.01, "last"))]
    scratch, gss = Guarded(dev, 1024), [Guarded(dev, 2) for _ in range(2 * len(xs))]
    for i, gs in enumerate(gss):                  # small, large, small, and once more: every launch has a result of its own
        x = xs[i % 3]
        awm.lib.wm_gscale_absmax(p(x), x.numel(), p(scratch.t), 12.0, p(gs.t), st())
    torch.cuda.synchronize()
    for i, gs in enumerate(gss):
        _scale_ok(np.float32((3.0, 700.0, 0.01)[i % 3]), 12, gs.np(), f"wm_gscale_absmax launch {i} in a row")
        assert gs.intact()


def test_gscale_clamp_ends(awm, dev):
    """gs is clamped to [1e-30, 1e30], ends that are no powers of two: only the clamp and gs (1 / gs) = 1 to an ulp are promised"""
    scratch = Guarded(dev, 1024)
    for m in Y.GS_CLAMP:
        x = to_dev(Y.absmax_input(8192, np.float32(m), "last"), dev)
        mx = to_dev(np.array([m], dtype=np.float32), dev)
        g2 = Guarded(dev, 2)
        awm.lib.wm_gscale_from_max(p(mx), 1, 12.0, p(g2.t), st())
        for gs in (_absmax(awm, x, 12, scratch), g2.np()):
            assert np.all(np.isfinite(gs)) and np.float32(1e-30) <= gs[0] <= np.float32(1e30), f"m = {m}: gs {gs[0]!r}"
            assert gs[0] in (np.float32(1e-30), np.float32(1e30)), f"m = {m}: the clamp is not reached"
            assert abs(float(gs[0]) * float(gs[1]) - 1.0) <= 2.0 ** -23


@pytest.mark.parametrize("n", Y.FROM_MAX_N)
def test_gscale_from_max(awm, dev, n):
    scratch = Guarded(dev, 1024)
    i = 0
    for L in Y.GS_L:
        for m in Y.gs_maxima():
            v = Y.dzmax_vector(m, n, ("first", "last")[i % 2])
            i += 1
            gs, vd = Guarded(dev, 2), to_dev(v, dev)
            awm.lib.wm_gscale_from_max(p(vd), n, float(L), p(gs.t), st())
            torch.cuda.synchronize()
            assert gs.intact()
            _scale_ok(m, L, gs.np(), f"wm_gscale_from_max n={n} m={m!r} L={L}")
            if n >= 4 and n % 4 == 0:             # the same scale as a pass over the tensor gives
                assert np.array_equal(gs.np(), _absmax(awm, vd, L, scratch))
    for bad in (0.0, float("inf"), float("nan")):
        v = np.full(n, bad, dtype=np.float32)
        gs, vd = Guarded(dev, 2), to_dev(v, dev)
        awm.lib.wm_gscale_from_max(p(vd), n, 12.0, p(gs.t), st())
        torch.cuda.synchronize()
        _scale_ok(np.float32(bad), 12, gs.np(), f"wm_gscale_from_max n={n} all {bad}")
    gs = Guarded(dev, 2)
    invalid(lambda: awm.lib.wm_gscale_from_max(p(scratch.t), 0, 12.0, p(gs.t), st()), gs)


@pytest.mark.parametrize("rows,row_len", Y.ROWS_CASES)
def test_absmax_rows(awm, dev, rows, row_len):
    r = Y.rng(700 + rows + row_len)
    x = Y.f32(r.uniform(-0.5, 0.5, (rows, row_len)))
    want = np.zeros(rows, dtype=np.float32)
    for row in range(min(rows, 3)):               # the maximum at the first element, at the last, and negative
        at = (0, row_len - 1, row_len // 2)[row]
        x[row, at] = (3.0, 5.0, -7.0)[row]
    if rows > 3:
        x[3, :] = -0.0                            # max |-0.0| is +0.0
        x[4, 1] = np.nan                          # a NaN row leaves its entry as the caller set it
        x[rows - 1, row_len - 1] = -9.0
    want = np.abs(x).max(axis=1)
    preset = np.zeros(rows, dtype=np.float32)
    if rows > 3:
        preset[4] = want[4] = 0.25
    out = Guarded(dev, rows, preset)
    xd = to_dev(x, dev)
    awm.lib.wm_absmax_rows(p(xd), rows, row_len, p(out.t), st())
    torch.cuda.synchronize()
    assert np.array_equal(out.np().view(np.int32), want.view(np.int32)), f"wm_absmax_rows ({rows}, {row_len})"
    assert out.intact()


def test_absmax_rows_invalid_arguments(awm, dev):
    x, out = torch.ones(64, device=dev), Guarded(dev, 4, np.zeros(4, dtype=np.float32))
    for rows, row_len in ((0, 4), (65536, 4), (1, 6), (1, 0)):
        invalid(lambda: awm.lib.wm_absmax_rows(p(x), rows, row_len, p(out.t), st()), out)
    invalid(lambda: awm.lib.wm_gscale_absmax(p(x), 6, p(x), 12.0, p(out.t), st()), out)
