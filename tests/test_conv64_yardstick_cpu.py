"""tests/conv64_yardstick.py without a GPU: its references against torch's float64 convolutions and autograd (to 1e-12), a numpy
restatement of each of the three arithmetics inside the derived bound in two accumulation orders, the same restatements with a defect
planted outside it, the builders' margins (no sample ever excluded), the mask layout, the scales, and the case tables against the
launch matrix."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv64_yardstick as Y
from yardstick_common import assert_within

SMALL = ((1, 8), (2, 132), (2, 260))


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    e = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert e <= 1e-12, f"{what}: {e:.3e}"


# --------------------------------------------------------------------------------------------------------- references against torch
@pytest.mark.parametrize("B,T", SMALL)
def test_conv1d_k3_forward_data_weight_and_bias_gradient(B, T):
    d = Y.conv_inputs(B, T, 3)
    x, w, b = (t64(d[k]).requires_grad_() for k in ("x", "w", "bias"))
    y = F.conv1d(x, w, b, padding=1)
    g = t64(d["e1"])
    y.backward(g)
    close(Y.conv_ref(d, 3, 0, 0, Y.EPI_BIAS)["y"], y.detach().numpy(), "Conv1d forward")
    close(Y.conv_ref(dict(d, x=d["e1"]), 3, 1, 0, Y.EPI_NONE)["y"], x.grad.numpy(), "Conv1d data gradient")
    r = Y.wgrad_ref(Y.f64(d["e1"]), Y.f64(d["x"]), 3, 0)
    close(r["dw"], w.grad.numpy(), "Conv1d weight gradient")
    close(r["dbias"], b.grad.numpy(), "Conv1d bias gradient")


@pytest.mark.parametrize("B,T", SMALL)
def test_conv_transpose_k7_forward_data_weight_and_bias_gradient(B, T):
    d = Y.conv_inputs(B, T, 7)
    x, w, b = (t64(d[k]).requires_grad_() for k in ("x", "w", "bias"))
    y = F.conv_transpose1d(x + t64(d["vec"])[:, :, None], w, b, padding=3)
    g = t64(d["e1"])
    y.backward(g)
    close(Y.conv_ref(d, 7, 2, Y.PRO_ADDVEC, Y.EPI_BIAS)["y"], y.detach().numpy(), "ConvTranspose1d forward")
    close(Y.conv_ref(dict(d, x=d["e1"]), 7, 3, 0, Y.EPI_NONE)["y"], x.grad.numpy(), "ConvTranspose1d data gradient")
    xin, _ = Y.pro_ref(Y.PRO_ADDVEC, d["x"], pa=d["vec"])
    r = Y.wgrad_ref(Y.f64(d["e1"]), xin, 7, 1)
    close(r["dw"], w.grad.numpy(), "ConvTranspose1d weight gradient [in][out][7]")
    close(r["dbias"], b.grad.numpy(), "ConvTranspose1d bias gradient")


def test_batchnorm_backward_prologue_and_relu_mask_as_a_graph():
    """conv2's data gradient of a ResBlock: z = conv2(h) with h = relu(y1 sc + sh); upstream of z is the BatchNorm backward
    A dz + B + C y2, with B as hi + lo.  dh masked by (y1 sc + sh > 0) is the launch (pro 3, epi 1); its sums are (sum, sum . y1)."""
    B, T = 2, 132
    d = Y.conv_inputs(B, T, 3)
    y1 = t64(d["e1"]).requires_grad_()
    sc, sh = t64(d["ea"])[None, :, None], t64(d["eb"])[None, :, None]
    w = t64(d["w"])
    z = F.conv1d(torch.relu(y1 * sc + sh), w, None, padding=1)
    up = t64(d["pa"])[None, :, None] * t64(d["x"]) + (t64(d["pb"][0]) + t64(d["pb"][1]))[None, :, None] + t64(d["pc"])[None, :, None] * t64(d["x2"])
    z.backward(up)
    want = (y1.grad / sc).numpy()                      # autograd's dy1 = dh (pre > 0) sc
    r = Y.conv_ref(d, 3, 1, Y.PRO_BNBWD, Y.EPI_RELUMASK)
    close(r["y"], want, "BatchNorm-backward prologue + ReLU mask")
    close(r["stats"][0], want.sum(axis=(0, 2)), "sum v")
    close(r["stats"][1], (want * Y.f64(d["e1"])).sum(axis=(0, 2)), "sum v e1")
    # the weight gradient with both prologues
    h = torch.relu(t64(d["e1"]) * sc + sh)
    wq = w.clone().requires_grad_()
    F.conv1d(h, wq, None, padding=1).backward(up)
    gp, _ = Y.pro_ref(Y.PRO_BNBWD, d["x"], d["x2"], d["pa"], d["pb"], d["pc"])
    xp, _ = Y.pro_ref(Y.PRO_BNRELU, d["e1"], pa=d["ea"], pb=d["eb"])
    close(Y.wgrad_ref(gp, xp, 3, 0)["dw"], wq.grad.numpy(), "weight gradient, gpro 3 / xpro 1")


def test_epilogues_and_eval_resblock():
    B, T = 2, 132
    d = Y.conv_inputs(B, T, 3)
    x, w, b, e1 = t64(d["x"]), t64(d["w"]), t64(d["bias"]), t64(d["e1"])
    acc = F.conv1d(x, w, None, padding=1)
    bb, ea, eb = b[None, :, None], t64(d["ea"])[None, :, None], t64(d["eb"])[None, :, None]
    want = {Y.EPI_ADD: acc + e1, Y.EPI_NONE: acc, Y.EPI_BNADDRELU: torch.relu(e1 + (acc + bb) * ea + eb), Y.EPI_BIASELU: F.elu(acc + bb),
            Y.EPI_BIASADDELU: F.elu(acc + bb + e1), Y.EPI_MULDELU: acc * torch.where(e1 > 0, torch.ones_like(e1), e1 + 1)}
    for epi, v in want.items():
        close(Y.conv_ref(d, 3, 0, 0, epi)["y"], v.numpy(), f"epilogue {epi}")
    r = Y.conv_ref(d, 3, 0, 0, Y.EPI_BIAS, stats=True)
    y = (acc + bb).numpy()
    close(r["stats"], np.stack([y.sum(axis=(0, 2)), (y * y).sum(axis=(0, 2))]), "BatchNorm sums of epi 0")
    r8 = Y.conv_ref(d, 3, 0, 0, Y.EPI_ADDSTATS)
    v8 = np.where(d["pmask"], acc.numpy() + np.where(d["gmask"], Y.f64(d["e1"]), 0.0), 0.0)
    close(r8["y"], v8, "epi 8")
    close(r8["stats"][1], (v8 * Y.f64(d["py2"])).sum(axis=(0, 2)), "epi 8 sum y ea")
    # the tail prologue
    xin, _ = Y.pro_ref(Y.PRO_TAIL, d["x"], d["x2"], d["pa"], d["pb"][0])
    close(xin, torch.relu(x + t64(d["x2"]) * t64(d["pa"])[None, :, None] + t64(d["pb"][0])[None, :, None]).numpy(), "tail prologue")
    # the fused eval ResBlock
    sc1, sh1, sc2, sh2 = d["pa"], d["pb"][0], d["ea"], d["eb"]
    w2 = Y.f32(Y.rng(5).standard_normal((64, 64, 3)) * 0.08)
    h = torch.relu((F.conv1d(x, w, b, padding=1)) * t64(sc1)[None, :, None] + t64(sh1)[None, :, None])
    ref = torch.relu(x + F.conv1d(h, t64(w2), t64(d["pc"]), padding=1) * t64(sc2)[None, :, None] + t64(sh2)[None, :, None])
    close(Y.resblock_eval_ref(d["x"], d["w"], d["bias"], sc1, sh1, w2, d["pc"], sc2, sh2, "bf")[0], ref.numpy(), "eval ResBlock")


def test_mask_layout_round_trip_and_bit_position():
    pos = Y.rng(1).random((2, 64, 36)) < 0.5
    words = Y.encode_mask(pos)
    assert words.shape == (128, 2) and np.array_equal(Y.decode_mask(words, 2, 36), pos)
    one = np.zeros((1, 64, 36), dtype=bool)
    one[0, 5, 33] = True
    w1 = Y.encode_mask(one)
    assert w1[5, 1] == 2 and w1.sum() == 2, "bit t % 32 of word t / 32 of row b * 64 + c"
    assert not (words[:, 1] >> 4).any(), "bits past T are clear"


def test_builders_exclude_no_sample():
    for B, T in SMALL + ((1, 4), (3, 132), (2, 384)):
        for kw in (3, 7):
            d = Y.conv_inputs(B, T, kw)
            assert Y.excluded_share(d) == 0.0
    assert Y.excluded_share(Y.conv_inputs(2, 192, 3, e1scale=3e4)) == 0.0 and Y.excluded_share(Y.conv_inputs(2, 192, 3, e1scale=1e-2)) == 0.0


def test_scales():
    for k in (-20, 0, 7):
        for m in (2.0 ** k, 2.0 ** k * (1 - 2.0 ** -24)):
            w = np.zeros((64, 64, 3), dtype=np.float32)
            w[3, 5, 1] = -m
            ws, inv = Y.weight_scale(w)
            assert 511.5 < float(np.float32(m)) * float(ws) <= 1023.0 and float(ws) * float(inv) == 1.0 and np.frexp(float(ws))[0] == 0.5
    assert Y.weight_scale(np.zeros((64, 64, 3)))[0] == 1.0
    assert Y.weight_scale(np.full((64, 64, 3), 1e-30))[0] == np.float32(1e30) and Y.weight_scale(np.full((64, 64, 3), 1e30))[0] == np.float32(2.0 ** -90)
    gs, inv = Y.grad_scale(3000.0, 12)
    assert gs == 1.0 and Y.grad_scale(2048.0, 12)[0] == 2.0 and Y.grad_scale(0.0, 12)[0] == 1.0


# ---------------------------------------------------------------------------------------------- restatements inside the bounds
def _launch_restated(arith, d, kw, mode, pro, epi, order, ws=1.0, gs=1.0, defect=None):
    """a forward / data-gradient launch in the kernels' number formats (epilogues 0, 1, 2, 3), with the defects that live in it"""
    W = Y.w_image(d["w"], mode)
    if defect == "no_flip":
        W = W[::-1]
    if defect == "swap_io":
        W = W.transpose(0, 2, 1)
    xin = Y.pro_restated(pro, d["x"], defect=defect, **Y.pro_args(pro, d))
    acc = Y.mm_restated(arith, W, xin, order, ws, gs)
    if defect in ("halo_left", "halo_right"):              # the column across the seam at t = 128 never reaches the tile next to it
        t, k, src = (128, 0, 127) if defect == "halo_left" else (127, 2, 128)
        acc[:, :, t] = Y.f32(Y.f64(acc[:, :, t]) - np.matmul(W[k], Y.f64(xin[:, :, src])[:, :, None])[:, :, 0])
    e1 = d["e1"]
    if epi == Y.EPI_BIAS:
        y = acc + d["bias"][None, :, None]
    elif epi == Y.EPI_RELUMASK:
        pre = Y.f32(Y.f64(e1) * Y.f64(d["ea"])[None, :, None] + Y.f64(d["eb"])[None, :, None])
        if defect == "mask_row":
            pre = np.roll(pre, 1, axis=1)
        y = np.where(pre > 0, acc, np.float32(0))
    elif epi == Y.EPI_ADD:
        y = acc + e1
    else:
        y = acc
    if defect == "ragged4":
        y = y.copy()
        y[:, :, -4:] = 0
    return y


def _tile_sums(y, e1, twice=None):
    """stats as the workgroups form them: float32 sums per 128-column tile, the tiles added in double"""
    s = np.zeros((2, 64))
    T = y.shape[2]
    tiles = [(b, t0) for b in range(y.shape[0]) for t0 in range(0, T, 128)]
    for i, (b, t0) in enumerate(tiles):
        a, q = y[b, :, t0:t0 + 128], (y[b, :, t0:t0 + 128] * e1[b, :, t0:t0 + 128])
        part = np.stack([a.sum(axis=1, dtype=np.float32), q.sum(axis=1, dtype=np.float32)]).astype(np.float64)
        s += part * (2 if twice == i else 1)
    return s


RESTATED = [(a, kw, mode, pro, epi) for a in Y.ARITHS for kw, mode, pro, epi in
            ((3, 0, 0, Y.EPI_BIAS), (3, 0, 1, Y.EPI_BIAS), (3, 1, 3, Y.EPI_RELUMASK), (3, 1, 3, Y.EPI_ADD), (7, 2, 2, Y.EPI_BIAS), (7, 3, 0, Y.EPI_NONE))]
WORST = {}


@pytest.mark.parametrize("arith,kw,mode,pro,epi", RESTATED)
def test_faithful_restatement_meets_the_bound(arith, kw, mode, pro, epi):
    for B, T in SMALL:
        d = Y.conv_inputs(B, T, kw)
        ws = float(Y.weight_scale(d["w"])[0]) if arith == "h" else 1.0
        xin, _ = Y.pro_ref(pro, d["x"], **Y.pro_args(pro, d))
        gs = float(Y.grad_scale(np.abs(xin).max(), 12)[0]) if arith == "h" and mode in (1, 3) else 1.0
        r = Y.conv_ref(d, kw, mode, pro, epi, arith, ws, gs)
        for order in (0, 1):
            y = _launch_restated(arith, d, kw, mode, pro, epi, order, ws, gs)
            assert_within(y, r["y"], r["bound"], f"{arith} kw {kw} mode {mode} pro {pro} epi {epi} ({B}, {T}) order {order}")
            WORST[arith] = max(WORST.get(arith, 0.0), float(np.max(np.abs(y - r["y"]) / np.maximum(r["bound"], 1e-300))))
            assert np.abs(y - r["y"]).max() <= 1e-6 * np.abs(r["y"]).max(), "the project's bar: 1e-6 of max |ref|"
            if epi == Y.EPI_RELUMASK:
                assert_within(_tile_sums(y, d["e1"]), r["stats"], r["stats_bound"], "stats")
    print("worst err/bound so far", WORST)


def test_bounds_are_not_vacuous():
    """a faithful restatement uses little of a worst-case gamma bound, so the bound is re-checked from the other side: a perturbation
    of ONE product term by 2^-12 of its size -- far below anything a wrong index produces -- already misses it"""
    d = Y.conv_inputs(2, 132, 3)
    for arith in Y.ARITHS:
        r = Y.conv_ref(d, 3, 0, 0, Y.EPI_NONE, arith)
        y = Y.mm_restated(arith, Y.w_image(d["w"], 0), d["x"], 0)
        assert np.all(np.abs(y - r["y"]) <= r["bound"])
        assert r["bound"].max() < 2.0 ** -12 * np.abs(Y.f64(d["w"])).max() * np.abs(Y.f64(d["x"])).max(), arith


# ------------------------------------------------------------------------------------------------------- planted defects miss them
def _misses(y, ref, bound):
    return bool(np.any(np.abs(Y.f64(y) - ref) > bound))


@pytest.mark.parametrize("arith", Y.ARITHS)
@pytest.mark.parametrize("defect,kw,mode,pro,epi,T", [
    ("halo_left", 3, 0, 0, Y.EPI_BIAS, 132), ("halo_right", 3, 0, 0, Y.EPI_BIAS, 132), ("ragged4", 3, 0, 0, Y.EPI_BIAS, 132),
    ("no_flip", 3, 1, 0, Y.EPI_NONE, 8), ("swap_io", 7, 2, 0, Y.EPI_BIAS, 8), ("no_pb_lo", 3, 1, 3, Y.EPI_ADD, 8), ("mask_row", 3, 1, 3, Y.EPI_RELUMASK, 8)])
def test_planted_defect_in_y_misses_the_bound(arith, defect, kw, mode, pro, epi, T):
    d = Y.conv_inputs(1, T, kw)
    ws = float(Y.weight_scale(d["w"])[0]) if arith == "h" else 1.0
    r = Y.conv_ref(d, kw, mode, pro, epi, arith, ws)
    good = _launch_restated(arith, d, kw, mode, pro, epi, 0, ws)
    bad = _launch_restated(arith, d, kw, mode, pro, epi, 0, ws, defect=defect)
    assert not _misses(good, r["y"], r["bound"])
    assert _misses(bad, r["y"], r["bound"]), f"{defect} passes the {arith} bound"


@pytest.mark.parametrize("arith", Y.ARITHS)
def test_planted_defects_in_the_side_outputs_miss_their_bounds(arith):
    B, T = 2, 260                                            # six 128-column tiles
    d = Y.conv_inputs(B, T, 3)
    ws = float(Y.weight_scale(d["w"])[0]) if arith == "h" else 1.0
    r = Y.conv_ref(d, 3, 1, Y.PRO_BNBWD, Y.EPI_RELUMASK, arith, ws)
    y = _launch_restated(arith, d, 3, 1, Y.PRO_BNBWD, Y.EPI_RELUMASK, 0, ws)
    assert not _misses(_tile_sums(y, d["e1"]), r["stats"], r["stats_bound"])
    assert _misses(_tile_sums(y, d["e1"], twice=5), r["stats"], r["stats_bound"]), "one tile counted twice in stats"
    # max |y|: the builder puts the largest |x| into the last quarter of the last row, so the largest |y| of a plain launch sits there
    r0 = Y.conv_ref(d, 3, 0, 0, Y.EPI_NONE, arith, ws)
    y0 = _launch_restated(arith, d, 3, 0, 0, Y.EPI_NONE, 0, ws)
    assert abs(float(np.abs(y0).max()) - r0["ymax"]) <= r0["ymax_bound"]
    assert abs(float(np.abs(y0[:, :16]).max()) - r0["ymax"]) > r0["ymax_bound"], "max |y| over one wave's quarter only"
    # dw with one tile missing; accumulate ignored
    gp = Y.pro_restated(Y.PRO_BNBWD, d["x"], d["x2"], d["pa"], d["pb"], d["pc"])
    g64, P = Y.pro_ref(Y.PRO_BNBWD, d["x"], d["x2"], d["pa"], d["pb"], d["pc"])
    prev = (Y.f32(Y.rng(3).standard_normal((64, 64, 3))), Y.f32(Y.rng(4).standard_normal(64)))
    rw = Y.wgrad_ref(g64, Y.f64(d["e1"]), 3, 0, arith, g_err=3 * Y.U * P, prev=prev)

    def dw_restated(skip=None, acc=True):
        img = np.zeros((3, 64, 64))
        for i, (b, t0) in enumerate((b, t0) for b in range(B) for t0 in range(0, T, 128)):
            if i == skip:
                continue
            gt = np.zeros_like(gp[b:b + 1])
            gt[:, :, t0:t0 + 128] = gp[b:b + 1, :, t0:t0 + 128]
            img += Y.wgrad_img(gt, d["e1"][b:b + 1], 3).astype(np.float32)
        dw = Y.f32(Y.dw_from_image(img, 0))
        return dw + prev[0] if acc else dw
    assert not _misses(dw_restated(), rw["dw"], rw["dw_bound"])
    assert _misses(dw_restated(skip=2), rw["dw"], rw["dw_bound"]), "one tile missing from dw"
    assert _misses(dw_restated(acc=False), rw["dw"], rw["dw_bound"]), "the accumulate bit ignored"


def test_gradient_scale_off_by_two_near_the_f16_maximum_misses_the_bound():
    """the gradient's largest element is brought to 40 000 by its scale (inside f16); twice that scale and it is clamped at 6e4"""
    d = Y.conv_inputs(1, 8, 7)
    d["x"] = Y.f32(d["x"] * 1e-3)
    d["x"][0, 3, 4] = 1.0
    gs = 40000.0 / 1.0
    gs = float(2.0 ** np.floor(np.log2(gs)))               # 32768: the maximum lands at 32768, its double is past f16
    ws = float(Y.weight_scale(d["w"])[0])
    r = Y.conv_ref(d, 7, 3, 0, Y.EPI_NONE, "h", ws, gs)
    assert not _misses(_launch_restated("h", d, 7, 3, 0, Y.EPI_NONE, 0, ws, gs), r["y"], r["bound"])
    assert _misses(_launch_restated("h", d, 7, 3, 0, Y.EPI_NONE, 0, ws, 2 * gs), r["y"], r["bound"])


# ------------------------------------------------------------------------------------------------------------------- the case tables
def test_cases_cover_the_launch_matrix():
    got = Y.covered()
    for entry, rows in Y.MATRIX.items():
        missing = [r for r in rows if r not in got[entry]]
        assert not missing, f"{entry}: no case row for {missing}"
    for shapes, mult in ((Y.SERIAL_SHAPES, 4), (Y.PIPE_SHAPES, 128), (Y.COL64_SHAPES, 64)):
        assert all(T % mult == 0 for _, T in shapes)
        tile = 64 if mult == 64 else 128
        ntiles = [B * -(-T // tile) for B, T in shapes]
        grids = [min(n, Y.KNUMCU) for n in ntiles]
        assert max(ntiles) > Y.KNUMCU, "no shape past the grid cap"
        assert any(g % 8 for g in grids) and any(g % 8 == 0 for g in grids), "both slot maps: identity, and across the XCDs"
