"""tests/bn_yardstick.py without a GPU.  For every case of its tables: the float32 restatement of the kernel's own formula meets the bound
that tests/test_gpu_bn_stack.py holds the kernel to (so the bound is attainable), the input conditions hold on the float64 reference (no
value within round-off of the ReLU's threshold, the constant channel's variance really negative, the partial sums exact), and the
restatement with one defect planted -- a dropped clamp, a biased running variance, row % B for row & 63, a mask shifted by a bit, Blo
dropped, accumulate ignored, a scale one binade off -- misses the bound.  Also: the exact-exponent scale formula of today against the
earlier log2f one over every float32 exponent."""
import numpy as np
import pytest
import torch

import bn_yardstick as Y
from yardstick_common import U, assert_within, ulp32


def within(a, ref, bound):
    """NaN is outside"""
    return bool(np.all(np.abs(np.asarray(a, dtype=np.float64) - ref) <= bound))


# --------------------------------------------------------------------------------------------------------------- wm_bn_finalize
@pytest.mark.parametrize("name,nparts,per_part,running", Y.FIN_CASES)
def test_finalize_restatement_meets_the_bound(name, nparts, per_part, running):
    inp = Y.finalize_inputs(nparts, per_part)
    assert inp["partials"].shape == (nparts, 2, 64) and inp["partials"].dtype == np.float32
    assert Y.sum_exact(inp["partials"])[1], "the double sum of the partials depends on its order"
    ref, got = Y.finalize_ref(inp, running), Y.finalize_restated(inp, running)
    for k in Y.FIN_NAMES:
        assert ref[k].dtype == np.float64 and np.all(np.isfinite(ref[k]))
        assert_within(got[k], ref[k], Y.finalize_bound(ref, k), f"{name} {k}")
    if per_part > 1:
        # the channel cases are what they claim
        assert ref["var_raw"][Y.CH_CONST] < -4.0 * Y.EPS, "the constant channel's float32 partials must give a negative variance"
        assert abs(ref["save_invstd"][Y.CH_CONST] - 1.0 / np.sqrt(Y.EPS)) <= ulp32(1.0 / np.sqrt(Y.EPS))
        assert ref["scale"][Y.CH_GAMMA0] == 0.0 and ref["shift"][Y.CH_GAMMA0] == float(inp["beta"][Y.CH_GAMMA0])
        assert ref["scale"][Y.CH_GAMMANEG] < 0.0
        ratio = abs(ref["save_mean"][Y.CH_OFFCENTRE]) * ref["save_invstd"][Y.CH_OFFCENTRE]
        assert 60.0 <= ratio <= 160.0, f"|mean| / std of the off-centre channel: {ratio}"
    if not running:
        assert np.array_equal(ref["running_mean"], inp["running_mean"].astype(np.float64))


def test_finalize_defects_miss_the_bound():
    tripped = {"no_clamp": 0, "biased": 0}
    for name, nparts, per_part, running in Y.FIN_CASES:
        inp = Y.finalize_inputs(nparts, per_part)
        ref = Y.finalize_ref(inp, running)
        for defect in tripped:
            got = Y.finalize_restated(inp, running, defect)
            bad = [k for k in Y.FIN_NAMES if not within(got[k], ref[k], Y.finalize_bound(ref, k))]
            if running and per_part > 1:
                if defect == "no_clamp":
                    assert "save_invstd" in bad and "scale" in bad and "running_var" in bad, (name, bad)
                    assert not np.isfinite(got["save_invstd"][Y.CH_CONST])
                elif per_part == 64:                      # at 256 * 16000 the unbiased factor is 1 + 2.4e-7: less than the bound
                    assert bad == ["running_var"], (name, bad)
            tripped[defect] += bool(bad)
    assert tripped["no_clamp"] >= 7 and tripped["biased"] >= 6


def test_finalize_count_one_and_big_count():
    one = Y.finalize_inputs(1, 1)
    assert one["count"] == 1.0
    ref = Y.finalize_ref(one)
    assert np.all(ref["var_raw"] == 0.0) and np.all(np.isfinite(ref["running_var"]))
    assert np.allclose(ref["running_var"], (1.0 - Y.MOMENTUM) * one["running_var"].astype(np.float64))
    assert Y.finalize_inputs(256, 16000)["count"] == 256.0 * 16000.0
    assert Y.NBT_START > 1 << 32
    assert Y.MOMENTUM == float(np.float32(0.1)) and Y.EPS == float(np.float32(1e-5))


# ------------------------------------------------------------------------------------------------------- wm_bn_eval_scale_shift
def test_eval_restatement_meets_the_bound():
    inp = Y.eval_inputs()
    assert set(np.unique(inp["running_var"])) == {np.float32(v) for v in Y.EVAL_RV}
    assert (inp["gamma"] < 0).any() and np.abs(inp["running_mean"]).max() > 1e3
    ref, got = Y.eval_ref(inp), Y.eval_restated(inp)
    for k in ("scale", "shift"):
        assert got[k].dtype == np.float32
        assert_within(got[k], ref[k], Y.eval_bound(ref, k), f"eval {k}")
    # a variance taken without eps (rv = 0 -> inf) or a root dropped is far outside
    assert not within(inp["gamma"] / (inp["running_var"] + np.float32(Y.EPS)), ref["scale"], Y.eval_bound(ref, "scale"))


# ------------------------------------------------------------------------------------------------------------------- the tail
@pytest.mark.parametrize("B", Y.TAIL_B)
@pytest.mark.parametrize("T", Y.TAIL_T)
def test_tail_inputs_margin_and_restatement(B, T):
    x, y, sc, sh = Y.tail_inputs(B, T)
    assert x.shape == y.shape == (B, 64, T) and x.dtype == y.dtype == sc.dtype == np.float32 and T % 4 == 0
    assert len(set(sc.tolist())) == 64 and len(set(sh.tolist())) == 64 and (sc < 0).any()
    t, r, big = Y.tail_terms(x, y, sc, sh)
    zeros = big == 0.0
    assert np.all(Y.tail_margin_ok(x, y, sc, sh)), "a reference value lies within round-off of the ReLU's threshold"
    assert np.all(np.abs(r[~zeros]) >= Y.MARGIN_ULPS * ulp32(big[~zeros]))
    assert zeros[:, Y.CH_ZEROS, ::7].all() and zeros.sum() == B * len(range(0, T, 7)) and np.all(r[zeros] == 0.0)
    out, pos, bound = Y.tail_ref(x, y, sc, sh)
    assert out.dtype == np.float64 and not pos[zeros].any() and pos.any() and (~pos).any()
    got, mask = Y.tail_restated(x, y, sc, sh)
    assert_within(got, out, bound, f"tail ({B}, {T}) out")
    assert np.all(got[~pos] == 0.0) and not np.signbit(got[~pos]).any()
    want = Y.pack_mask(pos)
    assert mask.shape == want.shape == (B * 64, (T + 31) // 32) and np.array_equal(mask, want)
    assert np.array_equal(Y.unpack_mask(want, T).reshape(B, 64, T), pos)
    if T % 32:
        assert not (want[:, -1] >> np.uint32(T % 32)).any(), "padding bits of the last dword"
    # the defects
    if B > 1:
        bad, _ = Y.tail_restated(x, y, sc, sh, "row_mod_B")
        assert not within(bad, out, bound), "row % B for row & 63 passes"
    _, shifted = Y.tail_restated(x, y, sc, sh, "mask_shift")
    assert not np.array_equal(shifted, want), "a mask shifted by one bit passes"


@pytest.mark.parametrize("B", Y.TAIL_B)
@pytest.mark.parametrize("T", Y.TAIL_T)
def test_reduce_inputs_and_restatement(B, T):
    x, y, sc, sh = Y.tail_inputs(B, T)
    _, pos, _ = Y.tail_ref(x, y, sc, sh)
    g = Y.reduce_inputs(B, T, pos)
    dz, dzmax, part, bound = Y.reduce_ref(g, y, pos)
    steps = Y.planted_steps(T)
    assert steps[0] < 4 and steps[1] >= T - 4 and steps[2] // 4 >= ((T // 4 - 1) // 1024) * 1024
    rows = np.arange(B * 64)
    assert np.array_equal(dzmax, (10.0 + rows / 100.0).astype(np.float32)), "the planted maximum of a set bit is the row's"
    assert np.array_equal(np.abs(dz).reshape(B * 64, T).argmax(axis=1), np.array(steps)[rows % 3])
    if T >= 36:
        assert (np.abs(g).reshape(B * 64, T).max(axis=1) == 20.0).sum() >= B * 8, "a larger |g| under a clear bit"
    assert part.dtype == np.float64 and part.shape == bound.shape == (B, 2, 64)
    d64 = dz.astype(np.float64)
    terms = np.stack([np.abs(d64).sum(axis=2), np.abs(d64 * y).sum(axis=2)], axis=1)
    assert Y.reduce_depth(T) == -(-(T // 4) // 256) + 12 and np.all(bound <= Y.gamma(T) * terms + Y.TINY), "never wider than gamma(T) sum |terms|"
    rdz, rmax, rpart = Y.reduce_restated(g, y, Y.pack_mask(pos))
    assert np.array_equal(rdz.view(np.int32), dz.view(np.int32)) and np.array_equal(rmax, dzmax)
    assert_within(rpart, part, bound, f"reduce ({B}, {T}) partial")
    sdz, smax, spart = Y.reduce_restated(g, y, (Y.pack_mask(pos) << np.uint32(1)).astype(np.uint32))
    assert not np.array_equal(sdz.view(np.int32), dz.view(np.int32)) and not within(spart, part, bound)


# ---------------------------------------------------------------------------------------------------------- wm_bn_bwd_finalize
@pytest.mark.parametrize("nparts,accumulate,eval_mode", Y.BWD_CASES)
def test_bwd_finalize_restatement_and_defects(nparts, accumulate, eval_mode):
    inp = Y.bwd_inputs(nparts)
    assert Y.sum_exact(inp["partials"])[1] and np.abs(inp["dgamma0"]).min() > 0 and np.abs(inp["dbeta0"]).min() > 0
    ref = Y.bwd_ref(inp, accumulate, eval_mode)
    got = Y.bwd_restated(inp, accumulate, eval_mode)
    for k in ("A", "C", "dgamma", "dbeta"):
        assert_within(got[k], ref[k], Y.bwd_bound(ref, k, accumulate), f"bwd {nparts} {accumulate} {eval_mode} {k}")
    assert np.all(np.abs(got["Blo"].astype(np.float64)) <= ulp32(got["Bhi"]) / 2)
    if eval_mode:                                 # the statistics are constants: dy = A dz, nothing sums to zero
        assert not got["C"].any() and not got["Bhi"].any() and not got["Blo"].any()
    else:
        res, mag = Y.zero_sum(inp, got["A"], got["C"], got["Bhi"], got["Blo"])
        print(f"zero sum: residue / (2^-45 of the terms) {np.max(res / (Y.ZERO_SUM * mag)):.3f}")
        assert np.all(mag > 0) and np.all(res <= Y.ZERO_SUM * mag)
        nb = Y.bwd_restated(inp, accumulate, eval_mode, "no_blo")
        res, mag = Y.zero_sum(inp, nb["A"], nb["C"], nb["Bhi"], nb["Blo"])
        assert not np.all(res <= Y.ZERO_SUM * mag), "Blo dropped passes"
    if accumulate:
        na = Y.bwd_restated(inp, accumulate, eval_mode, "no_accumulate")
        assert not within(na["dgamma"], ref["dgamma"], Y.bwd_bound(ref, "dgamma", 1))
        assert not within(na["dbeta"], ref["dbeta"], Y.bwd_bound(ref, "dbeta", 1))


def test_gscale_bwd_inputs_make_the_product_the_maximum():
    inp = Y.gscale_bwd_inputs()
    A = np.abs(inp["gamma"].astype(np.float64) * inp["save_invstd"].astype(np.float64))
    assert A[0] == 1.0 and np.all(A[1:] < 1.0) and np.all(np.abs(np.float32(A)[1:]) < 1.0)
    for nmax in Y.BWD_NMAX:
        for where in ("first", "last"):
            v = Y.dzmax_vector(np.float32(3.0), nmax, where)
            assert v.shape == (nmax,) and v.max() == 3.0 and (nmax == 1 or np.sort(v)[-2] < 1.5)


# ----------------------------------------------------------------------------------------------------------------- the scales
def test_scale_exact_puts_the_maximum_into_the_interval():
    for L in Y.GS_L:
        for m in Y.gs_maxima():
            gs = Y.scale_exact(m, L)
            assert Y.is_pow2(gs) and Y.in_interval(m, gs, L), (m, L, gs)
            assert float(Y.scale_frexp(m, L)) == gs
            assert not Y.in_interval(m, 2.0 * gs, L) and not Y.in_interval(m, 0.5 * gs, L), "a scale one binade off passes"
    for m in (0.0, np.inf, np.nan, -0.0):
        assert Y.scale_exact(m, 12) == 1.0 and float(Y.scale_frexp(m, 12)) == 1.0
    for m in Y.GS_CLAMP:
        gs = float(Y.scale_frexp(np.float32(m), 12))
        assert float(np.float32(1e-30)) <= gs <= float(np.float32(1e30)) and not Y.is_pow2(gs)


@pytest.mark.parametrize("L", Y.GS_L + (12.5, "512 / big"))
def test_exact_exponent_formula_against_the_log2f_formula(L):
    """Over every float32 exponent and 4099 mantissas (the ends, the 64 next to either end, random ones): the formula of today puts
    every maximum into the interval, and gives another scale than exp2f(floorf(L - log2f(m))) only where that one misses the interval
    -- which it does just above a power of two, where log2f(m) or L - log2f(m) rounds to the integer."""
    r = np.random.default_rng(5)
    frac = np.unique(np.concatenate([np.arange(65), (1 << 23) - 1 - np.arange(65), r.integers(0, 1 << 23, 3970)])).astype(np.uint32)
    exps = np.arange(1, 255, dtype=np.uint32)
    m = ((exps[:, None] << np.uint32(23)) | frac[None, :]).view(np.float32).reshape(-1)
    m = m[m < np.float32(3.0e38)]
    log2f_formula = Y.scale_log2f
    if L == "512 / big":                            # wm_bn_bwd_finalize's: the same interval as L = 9, through a quotient
        L, log2f_formula = 9, lambda m, L, clamp=True: Y.scale_log2f_div(m, clamp)
    new, old = Y.scale_frexp(m, L, clamp=False), log2f_formula(m, L, clamp=False)
    lo, hi = np.float32(1e-30), np.float32(1e30)
    free = (new > lo) & (new < hi)
    assert free.sum() > 0.7 * m.size
    assert np.all(Y.is_pow2(new[free])) and np.all(Y.in_interval(m[free], new[free], L)), "the formula of today misses the interval"
    differ = free & (new != old)
    # beyond the clamp both formulas end at the clamp, except in the binade next to it where the earlier one was a binade too large
    cn, co = Y.scale_frexp(m[~free], L), log2f_formula(m[~free], L)
    with np.errstate(over="ignore"):
        assert np.all(np.isin(cn, (lo, hi))) and np.all((cn == co) | (old[~free] == 2 * new[~free]))
    assert not np.any(Y.in_interval(m[differ], old[differ], L)), "a scale changed that was inside the interval"
    assert np.all(old[differ] == 2 * new[differ]), "where the two differ the earlier one is one binade too large"
    print(f"L = {L}: {int(differ.sum())} of {int(m.size)} maxima had a scale one binade too large; the largest relative distance "
          f"above a power of two: {float(np.max(np.frexp(m[differ])[0] * 2 - 1)) if differ.any() else 0.0:.2e}")
    if L == int(L) and log2f_formula is Y.scale_log2f:
        assert differ.any(), "the earlier formula shows no defect in numpy's float32: the restatement is not the kernel's"
        up = np.nextafter(np.float32(2.0 ** -20), np.float32(1))
        assert not Y.in_interval(up, Y.scale_log2f(up, L), L) and Y.in_interval(up, Y.scale_log2f(up, L, binade_off=-1), L)


def test_absmax_tables():
    assert Y.GS_N[-1] // 4 > 2048 * 1024 and all(n % 4 == 0 for n in Y.GS_N) and Y.GS_N[-1] * 4 < 35e6
    for rows, row_len in Y.ROWS_CASES:
        assert 1 <= rows <= 65535 and row_len % 4 == 0 and rows * row_len * 4 < 35e6
    x = Y.absmax_input(8196, np.float32(-3.0), "last")
    assert x[-1] == -3.0 and np.abs(x[:-1]).max() <= 1.5 and x.dtype == np.float32
    assert U == 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------ the producer chain
@pytest.mark.parametrize("B,T", Y.CHAIN_SHAPES)
@pytest.mark.parametrize("ratio", Y.CHAIN_RATIOS)
def test_chain_cases_are_off_centre_as_stated_and_the_float32_oracle_keeps_the_bar(ratio, B, T):
    off = Y.chain_offcentre(ratio, B, T)
    print(f"chain ratio {ratio} ({B}, {T}): |mean| / std of the BN1 input {off.min():.3f} ... {off.max():.3f}")
    assert np.all(np.abs(off - ratio) <= 1e-3 * max(ratio, 1))
    r64, r32 = Y.chain_ref(ratio, B, T)
    for name in Y.CHAIN_NAMES:
        assert r64[name].dtype == torch.float64 and r32[name].dtype == torch.float32 and float(r64[name].abs().max()) > 0
        floor = Y.chain_floor(name, ratio)
        e32 = Y.rel_err(r32[name], r64[name])
        print(f"  {name}: e32 {e32:.2e}, floor {floor:.2e}")
        # the float32 oracle (two-pass statistics) is well conditioned at every ratio: its bar never passes twice the floor
        assert 8.0 * e32 <= 2.0 * floor and Y.bar(r32[name], r64[name], floor) <= 2.0 * floor
    assert Y.chain_floor("block.1.running_var", 30) == 1e-5 * 901 and Y.chain_floor("block.4.running_var", 30) == 1e-5
    assert Y.chain_floor("block.1.weight", 3) == 2e-4 * 10 and Y.chain_floor("out", 30) == 1e-5 and Y.chain_floor("dx", 30) == 2e-4
