"""Every 64-to-64 convolution launch through its C ABI against the float64 yardsticks of tests/conv64_yardstick.py, one launch at a
time: wm_conv64_bf (phase-serial and pipelined kernels, bf16x6 and the f16 split), the native wm_conv64 / wm_wgrad64, wm_conv64_bf7 /
wm_wgrad64_bf7, wm_wgrad64_bf (both builds), wm_dwgrad64_bf with its stats / dw / dbias / dzmax side outputs, wm_resblock_eval_bf and
the wm_pack_w64_h* images.  Shapes are the smallest at which a path still differs: shorter than a halo, one tile plus a four-column
tile, a grid that is no multiple of 8 (identity slot map) and one that is (the map across the XCDs), interior seams, and 257 / 258 tiles
on the 256 workgroups of the persistent loop (a second trip, clamped prefetches, every stats / dzmax / slab slot in use).  Every output
and scratch buffer is Guarded, pre-filled with NaN and exactly as large as include/wm_hip.h says; every numeric comparison is
assert_within against a bound derived in the yardstick and prints its error / bound.  tests/test_conv64_yardstick_cpu.py shows a
restatement of each arithmetic meeting those bounds and a planted defect missing them."""
import numpy as np
import pytest
import torch

import conv64_yardstick as Y
from gpu_support import Guarded, awm, dev, invalid, p, st, to_dev  # noqa: F401
from yardstick_common import assert_within

pytestmark = pytest.mark.gpu

AR = {"bf": 0, "h": 1}
BAR = 1e-6                         # the project's existing bar (test_conv_bf16x6_is_fp32_grade): max error relative to max |ref|
SLAB3, SLAB7 = 3 * 4096 + 64, 7 * 4096 + 64


def mask_dev(pos, dev):
    return torch.from_numpy(Y.encode_mask(pos).view(np.int32)).to(dev)


def pack(awm, dev, w, kind, mode, row_scale=None):
    """the device image of w: kind "fp32" (wm_pack_w64), "bf" (wm_pack_w64_bf / _bf7 / _bf_scaled) or "h" (wm_pack_w64_h / _h7 / _h_scaled)"""
    kw = w.shape[2]
    wd = to_dev(w, dev)
    if kind == "fp32":
        img = Guarded(dev, kw * 4096)
        awm.lib.wm_pack_w64(p(wd), p(img.t), kw, mode, st())
    else:
        n = (3 if kind == "bf" else 2) * kw * 4096 + (4 if kind == "h" else 0)
        img = Guarded(dev, n // 2, dtype=torch.int32)
        name = "wm_pack_w64_" + kind + ("7" if kw == 7 else "")
        if row_scale is not None:
            rd = to_dev(row_scale, dev)
            getattr(awm.lib, name + "_scaled")(p(wd), p(rd), p(img.t), st())
        else:
            getattr(awm.lib, name)(p(wd), p(img.t), mode, st())
    torch.cuda.synchronize()
    assert img.intact(), "a weight image was written past its documented size"
    return img


class BarMiss(AssertionError):
    """the launch is inside its derived element-wise bound and misses only the project's bar of 1e-6 of max |ref|"""


MISSES = []


@pytest.fixture(autouse=True)
def _no_misses_yet():
    MISSES.clear()


def within_bar(got, ref, what):
    """noted now, judged by verdict() at the end of the test: every other comparison of the launch is made first"""
    e = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(float(np.abs(ref).max()), 1e-300))
    print(f"{what}: max err / max |ref| {e:.3e}")
    if e > BAR:
        MISSES.append(f"{what}: {e:.3e} of max |ref| is above the project's bar {BAR}")


def verdict():
    if MISSES:
        raise BarMiss("\n".join(MISSES))


# Findings, kept as strict expected failures (a BarMiss alone: a miss of a derived bound, a NaN or a touched canary still fails outright).
# Each launch below is inside its element-wise bound and above 1e-6 of max |ref| for a reason of its arithmetic:
#  - the f16 split holds an UNSCALED activation to an absolute 2^-25 (include/wm_hip.h), which at activations of 1e-2 is 3e-6 of them:
#    wm_conv64_bf arith 1 reaches 1.6e-6 of max |y| once the bias no longer dominates y (weights x 2^10), and the weight gradient of
#    wm_dwgrad64_bf and wm_wgrad64_bf7 arith 1, whose activation operand is unscaled, 1.07e-6 to 1.41e-6;
#  - seven taps are 448 products a sum: the native fp32 build reaches 1.01e-6 to 1.29e-6 and bf16x6 1.04e-6 at the shapes with the
#    most samples to take the maximum over (the bar was set on three taps).
def bar_miss(reason):
    return pytest.mark.xfail(strict=True, raises=BarMiss, reason=reason)


FLOOR_1E2 = "f16 split, activations x 1e-2: the absolute 2^-25 of the unscaled operand; measured {} of max |ref|"
TAPS7 = "seven taps, 448 products a sum; measured {} of max |ref|"
KNOWN_BAR_MISSES = {
    "conv64_bf_h_scales-0.01-1024.0": FLOOR_1E2.format("1.59e-6 (y)"),
    "7-0-0-False-129x132": TAPS7.format("1.01e-6 (native fp32)"),
    "7-2-0-False-129x132": TAPS7.format("1.29e-6 (native fp32)"),
    "7-0-3-False-2x260": TAPS7.format("1.10e-6 (native fp32)"),
    "pipe-bf-0-3-False-2x16512": TAPS7.format("1.04e-6 (bf16x6)"),
    "wgrad7_h_scales-1e-09-0.01": FLOOR_1E2.format("1.41e-6 (dw)"),
    "wgrad7_h_scales-1.0-0.01": FLOOR_1E2.format("1.29e-6 (dw)"),
    "wgrad7_h_scales-30000.0-0.01": FLOOR_1E2.format("1.25e-6 (dw)"),
    "dwgrad_h_scales-1-1-1e-09-0.01": FLOOR_1E2.format("1.07e-6 (dw)"),
    "dwgrad_h_scales-0-2-1.0-0.01": FLOOR_1E2.format("1.26e-6 (dw)"),
    "dwgrad_h_scales-0-2-30000.0-0.01": FLOOR_1E2.format("1.25e-6 (dw)"),
    "dwgrad_h_scales-0-8-1.0-0.01": FLOOR_1E2.format("1.26e-6 (dw)"),
    "dwgrad_h_scales-0-8-30000.0-0.01": FLOOR_1E2.format("1.25e-6 (dw)"),
}


def known(request, key):
    """the strict expected failure of a case of the table above (for the tests whose parameters come from stacked decorators)"""
    if key in KNOWN_BAR_MISSES:
        request.node.add_marker(bar_miss(KNOWN_BAR_MISSES[key]))


def flat(cases):
    """(row..., shapes) -> one parameter set per (row, shape)"""
    out = []
    for c in cases:
        for B, T in c[-1]:
            cid = "-".join(str(v) for v in c[:-1]) + f"-{B}x{T}"
            out.append(pytest.param(*c[:-1], B, T, id=cid, marks=[bar_miss(KNOWN_BAR_MISSES[cid])] if cid in KNOWN_BAR_MISSES else []))
    return out


def check_y(yg, r, what):
    got = yg.np(r["y"].shape)
    assert np.all(np.isfinite(got)), what + ": an element was not written (NaN) or is not finite"
    assert_within(got, r["y"], r["bound"], what + " y")
    within_bar(got, r["y"], what + " y")
    assert yg.intact(), what + ": a canary next to y changed"
    return got


def check_stats(sg, r, what):
    got = sg.np((Y.KNUMCU, 2, 64)).astype(np.float64)
    assert np.all(np.isfinite(got)), what + ": a stats slot is NaN (neither zeroed nor written)"
    assert_within(got.sum(axis=0), r["stats"], r["stats_bound"], what + " stats")
    assert sg.intact(), what + ": a canary next to stats changed"


def check_dw(dwg, dbg, r, what):
    assert_within(dwg.np(r["dw"].shape), r["dw"], r["dw_bound"], what + " dw")
    within_bar(dwg.np(r["dw"].shape), r["dw"], what + " dw")
    assert_within(dbg.np(), r["dbias"], r["dbias_bound"], what + " dbias")
    assert dwg.intact() and dbg.intact(), what + ": a canary next to dw / dbias changed"


def epi_args(epi, d, dev):
    """(bias, e1, ea, eb) device tensors or None, as the epilogue reads them"""
    bias = to_dev(d["bias"], dev) if epi in (0, 4, 5, 6) else None
    e1 = to_dev(d["e1"], dev) if epi in (1, 2, 4, 6, 7) else None
    ea, eb = (to_dev(d["ea"], dev), to_dev(d["eb"], dev)) if epi in (1, 4) else (None, None)
    return bias, e1, ea, eb


def pro_dev(pro, d, dev):
    a = Y.pro_args(pro, d)
    return tuple(to_dev(a[k], dev) if k in a else None for k in ("x2", "pa", "pb", "pc"))


def elu_output(d):
    """epi 7 reads e1 as an ELU OUTPUT (> -1): the builder's e1 through ELU"""
    d["e1"] = Y.f32(Y.elu(Y.f64(d["e1"])))
    return d


# ------------------------------------------------------------------------------------------------------------------- wm_conv64_bf
@pytest.mark.parametrize("kernel,arith,pro,epi,stats,B,T", flat(Y.CONV3_BF_CASES))
def test_conv64_bf(awm, dev, kernel, arith, pro, epi, stats, B, T):
    from awm_amd import ops
    d = Y.conv_inputs(B, T, 3)
    if epi == Y.EPI_MULDELU:
        elu_output(d)
    mode = 1 if pro == Y.PRO_BNBWD else 0
    ws = float(Y.weight_scale(d["w"])[0]) if arith == "h" else 1.0
    r = Y.conv_ref(d, 3, mode, pro, epi, arith, ws, stats=stats)
    img = pack(awm, dev, d["w"], arith, mode)
    x, (x2, pa, pb, pc), (bias, e1, ea, eb) = to_dev(d["x"], dev), pro_dev(pro, d, dev), epi_args(epi, d, dev)
    y, sg = Guarded(dev, B * 64 * T), Guarded(dev, Y.STATS_FLOATS)
    with ops.switches(schedule=0 if kernel == "serial" else 2):
        awm.lib.wm_conv64_bf(p(x), p(x2), p(img.t), p(pa), p(pb), p(pc), p(bias), p(e1), p(ea), p(eb), p(y.t), p(sg.t) if stats else None,
                             B, T, pro, epi, AR[arith], st())
        torch.cuda.synchronize()
    what = f"wm_conv64_bf {kernel} {arith} pro {pro} epi {epi} stats {stats} ({B}, {T})"
    got = check_y(y, r, what)
    if epi == Y.EPI_RELUMASK:
        assert not got[r["y"] == 0].view(np.int32).any(), what + ": +0.0 wherever the mask is clear"
    if stats:
        check_stats(sg, r, what)
    else:
        assert sg.intact(whole=True)
    verdict()


@pytest.mark.parametrize("wscale", Y.H_WSCALES)
@pytest.mark.parametrize("xscale", Y.H_XSCALES)
def test_conv64_bf_f16_split_scales(awm, dev, request, wscale, xscale):
    known(request, f"conv64_bf_h_scales-{xscale}-{wscale}")
    B, T = Y.MID_PIPE
    d = Y.conv_inputs(B, T, 3, wscale=0.08 * wscale, xscale=xscale)
    ws = float(Y.weight_scale(d["w"])[0])
    img = pack(awm, dev, d["w"], "h", 0)
    for pro in (0, 1):
        r = Y.conv_ref(d, 3, 0, pro, 0, "h", ws, stats=True)
        x, (x2, pa, pb, pc), bias = to_dev(d["x"], dev), pro_dev(pro, d, dev), to_dev(d["bias"], dev)
        y, sg = Guarded(dev, B * 64 * T), Guarded(dev, Y.STATS_FLOATS)
        awm.lib.wm_conv64_bf(p(x), None, p(img.t), p(pa), p(pb), None, p(bias), None, None, None, p(y.t), p(sg.t), B, T, pro, 0, 1, st())
        torch.cuda.synchronize()
        what = f"wm_conv64_bf h w x {wscale:g} x x {xscale:g} pro {pro}"
        check_y(y, r, what)
        check_stats(sg, r, what)
    verdict()


# ------------------------------------------------------------------------------------------------------- wm_conv64 (native fp32)
NATIVE_SHAPES = Y.SERIAL_SHAPES + ((257, 128),)            # 257 tiles for the 128- and the 256-column builds alike


@pytest.mark.parametrize("kw,pro,epi,stats,B,T", flat([c + (NATIVE_SHAPES,) for c in Y.CONV_NATIVE_CASES]))
def test_conv64_native(awm, dev, kw, pro, epi, stats, B, T):
    d = Y.conv_inputs(B, T, kw)
    mode = (1 if pro == Y.PRO_BNBWD else 0) if kw == 3 else (3 if epi == Y.EPI_NONE else 2)
    r = Y.conv_ref(d, kw, mode, pro, epi, "fp32", stats=stats)
    img = pack(awm, dev, d["w"], "fp32", mode)
    x, (x2, pa, pb, pc), (bias, e1, ea, eb) = to_dev(d["x"], dev), pro_dev(pro, d, dev), epi_args(epi, d, dev)
    y, sg = Guarded(dev, B * 64 * T), Guarded(dev, Y.STATS_FLOATS)
    awm.lib.wm_conv64(p(x), p(x2), p(img.t), p(pa), p(pb), p(pc), p(bias), p(e1), p(ea), p(eb), p(y.t), p(sg.t) if stats else None,
                      B, T, kw, pro, epi, st())
    torch.cuda.synchronize()
    what = f"wm_conv64 kw {kw} pro {pro} epi {epi} stats {stats} ({B}, {T})"
    check_y(y, r, what)
    if stats:
        check_stats(sg, r, what)
    else:
        assert sg.intact(whole=True)
    verdict()


def _wgrad_operands(d, gpro, xpro):
    """(g', x', g_err, x_err) in float64: the operands the weight gradient multiplies, and their prologues' rounding bounds"""
    g, Pg = Y.pro_ref(gpro, d["x"], **Y.pro_args(gpro, d))
    xa = dict(pa=d["ea"], pb=d["eb"]) if xpro == Y.PRO_BNRELU else (dict(pa=d["vec"]) if xpro == Y.PRO_ADDVEC else {})
    x, Px = Y.pro_ref(xpro, d["xw"], **xa)
    return g, x, Y.PRO_ROUNDINGS[gpro] * Y.U * Pg, Y.PRO_ROUNDINGS[xpro] * Y.U * Px


def _wgrad_dev(d, gpro, xpro, dev):
    g, (g2, ga, gb, gc) = to_dev(d["x"], dev), pro_dev(gpro, d, dev)
    x = to_dev(d["xw"], dev)
    xa = to_dev(d["ea"], dev) if xpro == 1 else (to_dev(d["vec"], dev) if xpro == 2 else None)
    xb = to_dev(d["eb"], dev) if xpro == 1 else None
    return g, g2, ga, gb, gc, x, xa, xb


def _prev(kw, seed=3):
    return Y.f32(Y.rng(seed).standard_normal((64, 64, kw))), Y.f32(Y.rng(seed + 1).standard_normal(64))


@pytest.mark.parametrize("kw,gpro,xpro,layout,B,T", flat([c + (NATIVE_SHAPES,) for c in Y.WGRAD_NATIVE_CASES]))
def test_wgrad64_native(awm, dev, kw, gpro, xpro, layout, B, T):
    d = Y.conv_inputs(B, T, kw)
    g64, x64, ge, xe = _wgrad_operands(d, gpro, xpro)
    args = _wgrad_dev(d, gpro, xpro, dev)
    for acc in (0, 1):
        prev = _prev(kw) if acc else None
        r = Y.wgrad_ref(g64, x64, kw, layout, "fp32", g_err=ge, x_err=xe, prev=prev)
        part = Guarded(dev, Y.PARTIAL_SLABS * (kw * 4096 + 64))
        dw, db = Guarded(dev, 64 * 64 * kw, prev[0] if acc else None), Guarded(dev, 64, prev[1] if acc else None)
        awm.lib.wm_wgrad64(*map(p, args), p(part.t), p(dw.t), p(db.t), B, T, kw, gpro, xpro, layout, acc, st())
        torch.cuda.synchronize()
        what = f"wm_wgrad64 kw {kw} gpro {gpro} xpro {xpro} layout {layout} accumulate {acc} ({B}, {T})"
        check_dw(dw, db, r, what)
        assert part.intact(), what + ": a slab was written past 256 x (KW * 4096 + 64) floats"
    verdict()


# ------------------------------------------------------------------------------------------- wm_conv64_bf7, wm_wgrad64_bf7 (7 taps)
def _conv7_cases():
    return flat([(k, a, pr, e, g, Y.PIPE_SHAPES if k == "pipe" else Y.SERIAL_SHAPES) for k, a, pr, e, g in Y.CONV7_CASES])


@pytest.mark.parametrize("kernel,arith,pro,epi,with_gs,B,T", _conv7_cases())
def test_conv64_bf7(awm, dev, kernel, arith, pro, epi, with_gs, B, T):
    d = Y.conv_inputs(B, T, 7)
    mode = 3 if epi == Y.EPI_NONE else 2
    ws = float(Y.weight_scale(d["w"])[0]) if arith == "h" else 1.0
    xin, _ = Y.pro_ref(pro, d["x"], **Y.pro_args(pro, d))
    gs = Y.grad_scale(np.float32(np.abs(xin).max()), 12) if with_gs else (np.float32(1), np.float32(1))
    r = Y.conv_ref(d, 7, mode, pro, epi, arith, ws, float(gs[0]))
    img = pack(awm, dev, d["w"], arith, mode)
    x, vec, bias = to_dev(d["x"], dev), to_dev(d["vec"], dev) if pro == 2 else None, to_dev(d["bias"], dev) if epi == 0 else None
    gsd = to_dev(np.array(gs, dtype=np.float32), dev) if with_gs else None
    y = Guarded(dev, B * 64 * T)
    awm.lib.wm_conv64_bf7(p(x), p(img.t), p(vec), p(bias), p(y.t), B, T, pro, epi, AR[arith], p(gsd), st())
    torch.cuda.synchronize()
    check_y(y, r, f"wm_conv64_bf7 {kernel} {arith} pro {pro} epi {epi} gscale {with_gs} ({B}, {T})")
    verdict()


@pytest.mark.parametrize("gfactor", Y.H_GSCALES)
@pytest.mark.parametrize("wscale", Y.H_WSCALES)
def test_conv64_bf7_f16_split_gradient_scales(awm, dev, gfactor, wscale):
    """the data-gradient launch of the ConvTranspose1d with its incoming gradient at 1e-9, 1 and 3e4 and one outlier 32 times the bulk"""
    B, T = Y.MID_PIPE
    d = Y.conv_inputs(B, T, 7, wscale=0.05 * wscale, xscale=gfactor, outlier=40.0)
    ws = float(Y.weight_scale(d["w"])[0])
    gs = Y.grad_scale(np.abs(d["x"]).max(), 12)
    r = Y.conv_ref(d, 7, 3, 0, Y.EPI_NONE, "h", ws, float(gs[0]))
    img, x, gsd = pack(awm, dev, d["w"], "h", 3), to_dev(d["x"], dev), to_dev(np.array(gs, dtype=np.float32), dev)
    y = Guarded(dev, B * 64 * T)
    awm.lib.wm_conv64_bf7(p(x), p(img.t), None, None, p(y.t), B, T, 0, 3, 1, p(gsd), st())
    torch.cuda.synchronize()
    check_y(y, r, f"wm_conv64_bf7 h data gradient g x {gfactor:g} w x {wscale:g}")
    verdict()


@pytest.mark.parametrize("arith,xpro,B,T", flat([c + (Y.PIPE_SHAPES[:5] + Y.SERIAL_SHAPES[:4],) for c in Y.WGRAD7_CASES]))
def test_wgrad64_bf7(awm, dev, arith, xpro, B, T):
    d = Y.conv_inputs(B, T, 7)
    g64, x64, ge, xe = _wgrad_operands(d, 0, xpro)
    gs = Y.grad_scale(np.abs(d["x"]).max(), 12) if arith == "h" else (np.float32(1), np.float32(1))
    g, x, vec = to_dev(d["x"], dev), to_dev(d["xw"], dev), to_dev(d["vec"], dev) if xpro == 2 else None
    gsd = to_dev(np.array(gs, dtype=np.float32), dev) if arith == "h" else None
    for acc in (0, 1):
        prev = _prev(7) if acc else None
        r = Y.wgrad_ref(g64, x64, 7, 1, arith, float(gs[0]), g_err=ge, x_err=xe, prev=prev)
        part = Guarded(dev, Y.PARTIAL_SLABS * SLAB7)
        dw, db = Guarded(dev, 64 * 64 * 7, prev[0] if acc else None), Guarded(dev, 64, prev[1] if acc else None)
        awm.lib.wm_wgrad64_bf7(p(g), p(x), p(vec), p(part.t), p(dw.t), p(db.t), B, T, xpro, acc, AR[arith], p(gsd), st())
        torch.cuda.synchronize()
        what = f"wm_wgrad64_bf7 {arith} xpro {xpro} accumulate {acc} ({B}, {T})"
        check_dw(dw, db, r, what)
        assert part.intact(), what + ": a slab was written past 256 x (7 * 4096 + 64) floats"
    verdict()


@pytest.mark.parametrize("xscale", Y.H_XSCALES)
@pytest.mark.parametrize("gfactor", Y.H_GSCALES)
def test_wgrad64_bf7_f16_split_scales(awm, dev, request, gfactor, xscale):
    """the ConvTranspose1d's weight gradient on the f16 split: the incoming gradient at 1e-9, 1 and 3e4 with one outlier 32 times the bulk
    (split under gs), the activation at 1e-2 and 30 (split unscaled)"""
    known(request, f"wgrad7_h_scales-{gfactor}-{xscale}")
    B, T = Y.MID_PIPE
    d = Y.conv_inputs(B, T, 7, xscale=gfactor, e1scale=xscale, outlier=40.0)
    g64, x64, ge, xe = _wgrad_operands(d, 0, 0)
    gs = Y.grad_scale(np.abs(d["x"]).max(), 12)
    g, x, gsd = to_dev(d["x"], dev), to_dev(d["xw"], dev), to_dev(np.array(gs, dtype=np.float32), dev)
    r = Y.wgrad_ref(g64, x64, 7, 1, "h", float(gs[0]), g_err=ge, x_err=xe)
    part, dw, db = Guarded(dev, Y.PARTIAL_SLABS * SLAB7), Guarded(dev, 64 * 64 * 7), Guarded(dev, 64)
    awm.lib.wm_wgrad64_bf7(p(g), p(x), None, p(part.t), p(dw.t), p(db.t), B, T, 0, 0, 1, p(gsd), st())
    torch.cuda.synchronize()
    check_dw(dw, db, r, f"wm_wgrad64_bf7 h g x {gfactor:g} act x {xscale:g}")
    assert part.intact()
    verdict()


# ------------------------------------------------------------------------------------------------------------------ wm_wgrad64_bf
@pytest.mark.parametrize("gpro,xpro,B,T", flat([c + (Y.COL64_SHAPES + ((1, 4), (3, 132)),) for c in Y.WGRAD3_BF_CASES]))
def test_wgrad64_bf(awm, dev, gpro, xpro, B, T):
    d = Y.conv_inputs(B, T, 3)
    g64, x64, ge, xe = _wgrad_operands(d, gpro, xpro)
    args = _wgrad_dev(d, gpro, xpro, dev)
    for acc in (0, 1, 2, 3):                          # bit 0: add to dw / dbias; bit 1: the output-split build where it exists
        prev = _prev(3) if acc & 1 else None
        r = Y.wgrad_ref(g64, x64, 3, 0, "bf", g_err=ge, x_err=xe, prev=prev)
        part = Guarded(dev, Y.PARTIAL_SLABS * SLAB3)
        dw, db = Guarded(dev, 64 * 64 * 3, prev[0] if acc & 1 else None), Guarded(dev, 64, prev[1] if acc & 1 else None)
        awm.lib.wm_wgrad64_bf(*map(p, args), p(part.t), p(dw.t), p(db.t), B, T, gpro, xpro, acc, st())
        torch.cuda.synchronize()
        what = f"wm_wgrad64_bf gpro {gpro} xpro {xpro} accumulate {acc} ({B}, {T})"
        check_dw(dw, db, r, what)
        assert part.intact(), what + ": a slab was written past 256 x (3 * 4096 + 64) floats"
    verdict()


# ----------------------------------------------------------------------------------------------------------------- wm_dwgrad64_bf
def _dwgrad(awm, dev, d, xpro, epi, gmask, arith, acc, what):
    """one wm_dwgrad64_bf launch on the builder's arrays (g = x, g2 = x2, ga / gb / gc = pa / pb / pc; the weight gradient's operand xw
    with ea / eb as its BatchNorm + ReLU; e1, ea, eb, py2, gmask, pmask as the epilogue reads them), every output against float64"""
    B, _, T = d["x"].shape
    h = arith == "h"
    ws = float(Y.weight_scale(d["w"])[0]) if h else 1.0
    gs = Y.grad_scale(np.float32(np.abs(d["pa"]).max()) * np.float32(np.abs(d["x"]).max()), 9) if h else (np.float32(1), np.float32(1))
    how = None if not gmask else ("x" if epi == Y.EPI_RELUMASK else "e1")
    r = Y.conv_ref(d, 3, 1, Y.PRO_BNBWD, epi, arith, ws, float(gs[0]), gmask=how)
    gx = np.where(d["gmask"], Y.f64(d["x"]), 0.0) if how == "x" else d["x"]
    g64, Pg = Y.pro_ref(Y.PRO_BNBWD, gx, **Y.pro_args(Y.PRO_BNBWD, d))
    x64, Px = Y.pro_ref(xpro, d["xw"], **(dict(pa=d["ea"], pb=d["eb"]) if xpro == 1 else {}))
    prev = _prev(3) if acc else None
    rw = Y.wgrad_ref(g64, x64, 3, 0, arith, float(gs[0]), g_err=3 * Y.U * Pg, x_err=Y.PRO_ROUNDINGS[xpro] * Y.U * Px, prev=prev)
    img = pack(awm, dev, d["w"], arith, 1)
    g, g2, ga, gb, gc = (to_dev(d[k], dev) for k in ("x", "x2", "pa", "pb", "pc"))
    x, e1 = to_dev(d["xw"], dev), to_dev(d["e1"], dev)
    xa, xb = (to_dev(d["ea"], dev), to_dev(d["eb"], dev)) if xpro == 1 else (None, None)
    if epi == Y.EPI_RELUMASK:
        ea, eb = to_dev(d["ea"], dev), to_dev(d["eb"], dev)
    elif epi == Y.EPI_ADDSTATS:
        ea, eb = to_dev(d["py2"], dev), mask_dev(d["pmask"], dev)
    else:
        ea, eb = None, None
    gm = mask_dev(d["gmask"], dev) if gmask else None
    gsd = to_dev(np.array(gs, dtype=np.float32), dev) if h else None
    has_stats = epi in (Y.EPI_RELUMASK, Y.EPI_ADDSTATS)
    y, sg, dzm = Guarded(dev, B * 64 * T), Guarded(dev, Y.STATS_FLOATS), Guarded(dev, Y.DZMAX_FLOATS)
    part = Guarded(dev, Y.PARTIAL_SLABS * SLAB3)
    dw, db = Guarded(dev, 64 * 64 * 3, prev[0] if acc else None), Guarded(dev, 64, prev[1] if acc else None)
    awm.lib.wm_dwgrad64_bf(p(g), p(g2), p(ga), p(gb), p(gc), p(img.t), p(x), p(xa), p(xb), p(e1), p(ea), p(eb), p(y.t),
                           p(sg.t) if has_stats else None, p(part.t), p(dw.t), p(db.t), B, T, xpro, epi, acc, p(gm), AR[arith], p(gsd),
                           p(dzm.t) if h else None, st())
    torch.cuda.synchronize()
    got = check_y(y, r, what)
    if has_stats:
        check_stats(sg, r, what)
        assert not got[r["y"] == 0].view(np.int32).any(), what + ": +0.0 wherever the mask is clear"
    else:
        assert sg.intact(whole=True)
    check_dw(dw, db, rw, what)
    assert part.intact(), what + ": a slab was written past 256 x (3 * 4096 + 64) floats"
    if h:
        m = dzm.np()
        grid = min(B * (T // 64), Y.KNUMCU)
        assert np.all(np.isfinite(m)), what + ": a dzmax slot is NaN (neither zeroed nor written)"
        assert not m[grid:].view(np.int32).any(), what + ": a dzmax slot beyond the grid is not +0.0"
        assert np.float32(m.max()).view(np.int32) == np.float32(np.abs(got).max()).view(np.int32), what + ": max dzmax is not max |y| as written"
        assert abs(float(m.max()) - r["ymax"]) <= r["ymax_bound"], what + ": dzmax is outside the element bound of the reference's max |y|"
        assert dzm.intact()
    else:
        assert dzm.intact(whole=True)


@pytest.mark.parametrize("xpro,epi,gmask,arith,B,T", flat([c + (Y.COL64_SHAPES,) for c in Y.DWGRAD_CASES]))
def test_dwgrad64_bf(awm, dev, xpro, epi, gmask, arith, B, T):
    d = Y.conv_inputs(B, T, 3)
    acc = (B + T // 64) & 1                            # accumulate 0 and 1 alternate over the shapes; both at the mid shape below
    _dwgrad(awm, dev, d, xpro, epi, gmask, arith, acc, f"wm_dwgrad64_bf xpro {xpro} epi {epi} gmask {gmask} {arith} accumulate {acc} ({B}, {T})")
    if (B, T) == Y.MID_COL64:
        _dwgrad(awm, dev, d, xpro, epi, gmask, arith, 1 - acc, f"wm_dwgrad64_bf xpro {xpro} epi {epi} gmask {gmask} {arith} accumulate {1 - acc} ({B}, {T})")
    verdict()


@pytest.mark.parametrize("xscale", Y.H_XSCALES)
@pytest.mark.parametrize("gfactor", Y.H_GSCALES)
@pytest.mark.parametrize("wscale", Y.H_WSCALES)
@pytest.mark.parametrize("xpro,epi", [(1, 1), (0, 2), (0, 8)])
def test_dwgrad64_bf_f16_split_scales(awm, dev, request, xpro, epi, wscale, gfactor, xscale):
    """incoming gradient at 1e-9, 1 and 3e4 with one outlier 32 times the bulk, weights at 2^-20, 1 and 2^10, activations at 1e-2 and
    30: the scale gs puts max |A| max |dz| at 2^9, and what dzmax hands to the next launch is max |y| exactly"""
    known(request, f"dwgrad_h_scales-{xpro}-{epi}-{gfactor}-{xscale}")        # at every scale of the weights: a power of two, exact
    B, T = Y.MID_COL64
    d = Y.conv_inputs(B, T, 3, wscale=0.08 * wscale, xscale=gfactor, cscale=gfactor, e1scale=xscale, outlier=40.0)
    if epi != Y.EPI_RELUMASK:                          # e1 is a gradient there, not an activation
        d["e1"] = Y.f32(d["e1"] * np.float32(gfactor * wscale / xscale))
    _dwgrad(awm, dev, d, xpro, epi, True, "h", 0, f"wm_dwgrad64_bf h xpro {xpro} epi {epi} g x {gfactor:g} w x {wscale:g} act x {xscale:g}")
    verdict()


# ------------------------------------------------------------------------------------------------------------ wm_resblock_eval_bf
@pytest.mark.parametrize("arith", ("bf", "h"))
@pytest.mark.parametrize("B,T", Y.SERIAL_SHAPES)
def test_resblock_eval_bf(awm, dev, arith, B, T):
    d = Y.conv_inputs(B, T, 3)
    w2 = Y.f32(Y.rng(5 + T).standard_normal((64, 64, 3)) * 0.08)
    sc1, sh1, sc2, sh2 = d["pa"], d["pb"][0], d["ea"], d["eb"]
    i1, i2 = pack(awm, dev, d["w"], arith, 0, sc1), pack(awm, dev, w2, arith, 0, sc2)
    x, b1d, b2d, sc1d, sh1d, sc2d, sh2d = (to_dev(a, dev) for a in (d["x"], d["bias"], d["pc"], sc1, sh1, sc2, sh2))
    for biases in (True, False):
        b1, b2 = (d["bias"], d["pc"]) if biases else (None, None)
        ref, bound = Y.resblock_eval_ref(d["x"], d["w"], b1, sc1, sh1, w2, b2, sc2, sh2, arith)
        y = Guarded(dev, B * 64 * T)
        awm.lib.wm_resblock_eval_bf(p(x), p(i1.t), p(i2.t), p(b1d) if biases else None, p(sc1d), p(sh1d), p(b2d) if biases else None, p(sc2d), p(sh2d),
                                    p(y.t), B, T, AR[arith], st())
        torch.cuda.synchronize()
        check_y(y, dict(y=ref, bound=bound), f"wm_resblock_eval_bf {arith} biases {biases} ({B}, {T})")
    verdict()


# ----------------------------------------------------------------------------------------------------------------- wm_pack_w64_h*
def _pack_weights(kw):
    """(name, weight): all zero; a maximum of 2^k and of 2^k (1 - 2^-24) among smaller ones; 1e-30 and 1e30"""
    r = Y.rng(40 + kw)
    base = Y.f32(r.uniform(-0.4, 0.4, (64, 64, kw)))
    out = [("zero", np.zeros((64, 64, kw), dtype=np.float32)), ("1e-30", Y.f32(base * 2.5e-30)), ("1e30", Y.f32(base * 2.5e30))]
    for k in (-20, 0, 10):
        for name, m in ((f"2^{k}", 2.0 ** k), (f"2^{k}(1-2^-24)", 2.0 ** k * (1 - 2.0 ** -24))):
            w = Y.f32(base * np.float32(2.0 ** k))
            w[5, 9, kw - 1] = -m
            out.append((name, w))
    return out


@pytest.mark.parametrize("kw,scaled", [(3, False), (3, True), (7, False)])
def test_pack_w64_h_images(awm, dev, kw, scaled):
    row = Y.f32(2.0 ** Y.rng(2).integers(-2, 3, 64)) if scaled else None     # powers of two: w row_scale is exact
    for name, w in _pack_weights(kw):
        for mode in ((0,) if scaled else ((0, 1) if kw == 3 else (2, 3))):
            img = pack(awm, dev, w, "h", mode, row)
            raw = img.t.cpu().numpy().view(np.uint16)
            val, ws, inv = Y.decode_h_image(raw, kw)
            want_ws, want_inv = Y.weight_scale(w, row)
            what = f"wm_pack_w64_h{'7' if kw == 7 else ''}{'_scaled' if scaled else ''} {name} mode {mode}"
            assert ws.view(np.int32) == want_ws.view(np.int32) and inv.view(np.int32) == want_inv.view(np.int32), \
                f"{what}: {{ws, 1 / ws}} = {{{ws!r}, {inv!r}}}, documented {{{want_ws!r}, {want_inv!r}}}"
            v = Y.w_image(Y.f64(w) * (Y.f64(row)[:, None, None] if scaled else 1.0), mode) * float(ws)
            # x = v ws is one float32 product (exact while ws is a power of two, not at the clamp's ends), then 11 + 11 bits and the floor
            assert_within(val, v, (Y.U + 2.0 ** -22) * np.abs(v) + Y.FLOOR_H, what + " hi + lo")


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(awm, dev):
    from awm_amd import ops
    L = awm.lib
    B, T = 1, 128
    d = Y.conv_inputs(B, T, 3)
    f = to_dev(d["x"], dev)                            # any readable frame / vector: a refused call reads nothing
    img = Guarded(dev, 3 * 3 * 4096, dtype=torch.int32)
    y, sg, dzm = Guarded(dev, B * 64 * T), Guarded(dev, Y.STATS_FLOATS), Guarded(dev, Y.DZMAX_FLOATS)
    part, dw, db = Guarded(dev, Y.PARTIAL_SLABS * SLAB7), Guarded(dev, 64 * 64 * 7), Guarded(dev, 64)
    outs = (y, sg, dzm, part, dw, db, img)
    q = p(f)

    def conv_bf(pro, epi, stats, arith, T_=T):
        return lambda: L.wm_conv64_bf(q, q, p(img.t), q, q, q, q, q, q, q, p(y.t), p(sg.t) if stats else None, B, T_, pro, epi, arith, st())
    # unsupported (pro, epi, stats) under both schedules; arith 1 outside its matrix, at T % 128 != 0 and under schedule 0; arith 2; T % 4
    for sched in (0, 2):
        with ops.switches(schedule=sched):
            for pro, epi, stats in ((3, 1, False), (3, 2, True), (3, 3, True), (3, 0, False), (1, 1, True), (2, 0, False), (0, 5, True), (0, 8, False),
                                    (1, 5, False), (4, 0, True), (0, 9, False)):
                invalid(conv_bf(pro, epi, stats, 0), *outs)
            invalid(conv_bf(1, 4, True, 0), *outs)
            invalid(conv_bf(0, 0, False, 2), *outs)
            invalid(conv_bf(0, 0, False, 0, 126), *outs)
            invalid(conv_bf(0, 0, False, 1, 132), *outs)
            for pro, epi, stats in ((3, 1, True), (3, 2, False), (0, 2, False), (0, 5, False), (1, 4, True)):
                invalid(conv_bf(pro, epi, stats, 1), *outs)
    with ops.switches(schedule=0):
        invalid(conv_bf(0, 0, False, 1), *outs)
        invalid(conv_bf(1, 4, False, 0), *outs)       # the fused inference epilogue exists in the pipelined kernel only
    # native
    for kw, pro, epi, stats in ((3, 3, 1, False), (3, 0, 2, False), (7, 0, 0, True), (7, 1, 0, False), (7, 2, 3, False), (5, 0, 0, False), (3, 0, 4, False)):
        invalid(lambda: L.wm_conv64(q, q, q, q, q, q, q, q, q, q, p(y.t), p(sg.t) if stats else None, B, T, kw, pro, epi, st()), *outs)
    invalid(lambda: L.wm_conv64(q, q, q, q, q, q, q, q, q, q, p(y.t), None, B, 130, 3, 0, 0, st()), *outs)
    for kw, gpro, xpro in ((3, 0, 0), (3, 0, 1), (3, 3, 2), (7, 3, 0), (7, 0, 1), (5, 0, 0)):
        invalid(lambda: L.wm_wgrad64(q, q, q, q, q, q, q, q, p(part.t), p(dw.t), p(db.t), B, T, kw, gpro, xpro, 0, 0, st()), *outs)
    invalid(lambda: L.wm_wgrad64(q, q, q, q, q, q, q, q, p(part.t), p(dw.t), p(db.t), B, 130, 3, 3, 1, 0, 0, st()), *outs)
    # 7 taps
    for pro, epi, arith, T_ in ((1, 0, 0, T), (2, 3, 0, T), (0, 1, 0, T), (0, 0, 2, T), (0, 0, 1, 132), (1, 0, 1, T), (0, 0, 0, 130)):
        invalid(lambda: L.wm_conv64_bf7(q, p(img.t), q, q, p(y.t), B, T_, pro, epi, arith, None, st()), *outs)
    for xpro, arith, gsc, T_ in ((1, 0, None, T), (3, 0, None, T), (0, 2, None, T), (0, 1, None, T), (0, 0, None, 130)):
        invalid(lambda: L.wm_wgrad64_bf7(q, q, q, p(part.t), p(dw.t), p(db.t), B, T_, xpro, 0, arith, gsc, st()), *outs)
    # k3 weight gradient
    for gpro, xpro, acc, T_ in ((0, 1, 0, T), (3, 2, 0, T), (1, 0, 0, T), (0, 1, 2, T), (3, 1, 0, 130)):
        invalid(lambda: L.wm_wgrad64_bf(q, q, q, q, q, q, q, q, p(part.t), p(dw.t), p(db.t), B, T_, gpro, xpro, acc, st()), *outs)
    # data + weight gradient: unsupported forms, T % 64, a required null pointer, arith 2, arith 1 without its scale
    m = torch.zeros(B * 64 * (T // 32), dtype=torch.int32, device=dev)

    def dwg(xpro, epi, stats, gm, arith, gsc, T_=T, g=q, wp=p(img.t), yy=p(y.t), pt=p(part.t), dww=p(dw.t), ea=q, eb=q):
        return lambda: L.wm_dwgrad64_bf(g, q, q, q, q, wp, q, q, q, q, ea, eb, yy, p(sg.t) if stats else None, pt, dww, p(db.t), B, T_, xpro, epi, 0,
                                        p(m) if gm else None, arith, gsc, p(dzm.t), st())
    for a in (dwg(1, 1, False, True, 0, None), dwg(0, 1, True, True, 0, None), dwg(1, 2, False, True, 0, None), dwg(0, 2, True, True, 0, None),
              dwg(0, 8, True, False, 0, None), dwg(0, 8, False, True, 0, None), dwg(0, 3, False, False, 0, None), dwg(0, 2, False, False, 2, q),
              dwg(0, 2, False, False, 1, None), dwg(0, 2, False, False, 0, None, 96), dwg(0, 2, False, False, 0, None, 132),
              dwg(0, 2, False, False, 0, None, g=None), dwg(0, 2, False, False, 0, None, wp=None), dwg(0, 2, False, False, 0, None, yy=None),
              dwg(0, 2, False, False, 0, None, pt=None), dwg(0, 2, False, False, 0, None, dww=None), dwg(1, 1, True, True, 0, None, ea=None),
              dwg(0, 8, True, True, 0, None, eb=None)):
        invalid(a, *outs)
    # inference ResBlock
    for kwargs in (dict(T_=130), dict(arith=2), dict(x=None), dict(w1=None), dict(sc=None), dict(yy=None)):
        a = dict(T_=T, arith=0, x=q, w1=p(img.t), sc=q, yy=p(y.t))
        a.update(kwargs)
        invalid(lambda: L.wm_resblock_eval_bf(a["x"], a["w1"], p(img.t), q, a["sc"], q, q, q, q, a["yy"], B, a["T_"], a["arith"], st()), *outs)
    # pack modes out of range, required null pointers
    for name, modes in (("wm_pack_w64_bf", (-1, 2)), ("wm_pack_w64_h", (-1, 2, 3)), ("wm_pack_w64_bf7", (0, 1, 4)), ("wm_pack_w64_h7", (0, 1, 4))):
        for mode in modes:
            invalid(lambda: getattr(L, name)(q, p(img.t), mode, st()), *outs)
    for kw, mode in ((3, -1), (3, 4), (5, 0)):
        invalid(lambda: L.wm_pack_w64(q, p(y.t), kw, mode, st()), *outs)
    invalid(lambda: L.wm_pack_w64_h(None, p(img.t), 0, st()), *outs)
    invalid(lambda: L.wm_pack_w64_h(q, None, 0, st()), *outs)
    invalid(lambda: L.wm_pack_w64_h_scaled(q, None, p(img.t), st()), *outs)
    invalid(lambda: L.wm_pack_w64_bf_scaled(q, None, p(img.t), st()), *outs)
