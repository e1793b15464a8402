"""The gradient frame behind the Generator's Conv1d(64, 1, 1) head, dout[b,c,t] = hw[c] g1[b,t], formed on load by its three readers
(wm_relu_bwd_reduce_mask_r1, wm_dwgrad64_bf_r1 as conv2 pair and as conv1 pair) instead of written by wm_head1_bwd and read back.
In every test the reference is the launch sequence the route replaces, run in the same test: wm_head1_bwd with dx, then
wm_relu_bwd_reduce_mask and wm_dwgrad64_bf on the materialised frame.  Every comparison is bit for bit: the frame element is one
fp32 multiply on both routes and no sum is regrouped, so there is no tolerance anywhere in this file."""
import copy

import pytest
import torch

from gpu_support import awm, dev  # noqa: F401
from gpu_support import _spy, bits, p, reference_models, rnd, same, st
from oracle import wm_oracle as O

pytestmark = pytest.mark.gpu

NCU = 256
SCALES = [1e-6, 1.0, 3e3]          # of the upstream gradient: max |dz| -> the f16 split's power-of-two scale moves with it
INVALID = 1                        # hipErrorInvalidValue


def eq(a, b, what):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), f"{what}: differs from the frame route"


def upstream(B, T, scale, dev):
    """g1 [B,1,T] and hw [1,64,1]: mixed signs, exact zeros at every 7th step, the last clip (of more than one) all zero"""
    g1 = rnd(B, 1, T, seed=41 + T) * scale
    g1[:, :, ::7] = 0.0
    if B > 1:
        g1[B - 1] = 0.0
    hw = rnd(1, 64, 1, seed=42, scale=0.2)
    assert bool((g1 > 0).any()) and bool((g1 < 0).any()) and bool((hw > 0).any()) and bool((hw < 0).any())
    return g1.to(dev), hw.to(dev)


def block_frames(lib, B, T, dev):
    """x, y1, y2 of a ResBlock, its folded BatchNorm constants and the sign bits of out = relu(x + y2*sc2 + sh2) (both bit values,
    exact zeros in channel 5 that are not clamped negatives), as frames() of test_gpu_tail_in_head.py builds them"""
    x, y2, y1 = rnd(B, 64, T, seed=11 + T), rnd(B, 64, T, seed=12 + T), rnd(B, 64, T, seed=15 + T)
    sc2, sh2 = rnd(64, seed=13).abs() + 0.5, rnd(64, seed=14, scale=0.3)
    sh2[5] = 0.0
    x[:, 5, ::7] = 0.0
    y2[:, 5, ::7] = 0.0
    x, y1, y2, sc2, sh2 = (t.to(dev) for t in (x, y1, y2, sc2, sh2))
    out = torch.empty_like(x)
    mask = torch.full((B * 64 * ((T + 31) // 32),), -1, dtype=torch.int32, device=dev)
    lib.wm_bn_add_relu_mask(p(x), p(y2), p(sc2), p(sh2), p(out), p(mask), B, T, st())
    assert bool((out == 0).any()) and bool((out > 0).any())
    sc1, sh1 = (rnd(64, seed=16).abs() + 0.5).to(dev), rnd(64, seed=17, scale=0.3).to(dev)
    return dict(x=x, y1=y1, y2=y2, out=out, mask=mask, sc1=sc1, sh1=sh1)


def head1_bwd(lib, g1, out, hw, with_dx):
    B, _, T = out.shape
    dx = torch.full_like(out, float("nan")) if with_dx else None
    part = torch.full((1024 * 65,), float("nan"), device=out.device)
    dw, db = torch.full_like(hw, float("nan")), torch.full((1,), float("nan"), device=out.device)
    lib.wm_head1_bwd(p(g1), p(out), p(hw), p(dx), p(part), p(dw), p(db), B, T, 0, st())
    return dx, dw, db


def bn_stats(dev, seed):
    """(gamma, saved mean, saved invstd) of a BatchNorm1d(64) off its trivial values"""
    return ((rnd(64, seed=seed).abs() + 0.5).to(dev), rnd(64, seed=seed + 1, scale=0.1).to(dev), (rnd(64, seed=seed + 2).abs() + 0.5).to(dev))


def finalize(lib, part, nparts, n, bn, dzmax, nmax, dev):
    """wm_bn_bwd_finalize -> (k [4,64] = A, B hi, B lo, C; gscale [2])"""
    gamma, mu, inv = bn
    k, gs = torch.empty(4, 64, device=dev), torch.empty(2, device=dev)
    dg, dbe = torch.empty(64, device=dev), torch.empty(64, device=dev)
    lib.wm_bn_bwd_finalize(p(part), nparts, n, p(gamma), p(mu), p(inv), p(k[0]), p(k[1]), p(k[3]), p(dg), p(dbe), 0, 0, p(dzmax), nmax, p(gs), st())
    return k, gs


# ------------------------------------------------------------------------------- 1. wm_head1_bwd without dx
# (2, 64), (3, 200), (2, 1088), (5, 8192): one trip of the grid-stride loop each (total4 = B T / 4 <= 10240, and the grid is
# min(ceil(total4 / 256), 1024) workgroups of 256 threads).  The second trip needs total4 > 1024 * 256 = 262144, which none of those
# reaches, so HEAD1_TWO_TRIPS adds the smallest-but-one such shape: total4 = 270336, the first 32 workgroups run the loop twice.
HEAD1_SHAPES = [(2, 64), (3, 200), (2, 1088), (5, 8192)]
HEAD1_TWO_TRIPS = (33, 32768)


@pytest.mark.parametrize("B,T", HEAD1_SHAPES + [HEAD1_TWO_TRIPS])
def test_head1_bwd_without_dx(awm, dev, B, T):
    lib = awm.lib
    if B * T > 1 << 20:              # the large frame: one random clip on the device, a different gain per clip
        out = (rnd(1, 64, T, seed=21 + T).to(dev) * torch.arange(1, B + 1, device=dev)[:, None, None]).clamp_(min=0)
    else:
        out = rnd(B, 64, T, seed=21 + T).clamp_(min=0).to(dev)
    for scale in SCALES:
        g1, hw = upstream(B, T, scale, dev)
        dx, dw_ref, db_ref = head1_bwd(lib, g1, out, hw, True)
        _, dw, db = head1_bwd(lib, g1, out, hw, False)
        eq(dw, dw_ref, "dw")
        eq(db, db_ref, "db")
        eq(dx, hw * g1, "the frame itself is the one multiply")


# ------------------------------------------------------------------------------- 2. the reduction pass
@pytest.mark.parametrize("B,T", [(2, 64), (3, 200), (2, 1088)])
@pytest.mark.parametrize("scale", SCALES)
def test_relu_bwd_reduce_mask_r1(awm, dev, B, T, scale):
    lib = awm.lib
    f = block_frames(lib, B, T, dev)
    g1, hw = upstream(B, T, scale, dev)
    frame, _, _ = head1_bwd(lib, g1, f["out"], hw, True)
    res = []
    for r1 in (False, True):
        part, dzm = torch.full((B * 128,), float("nan"), device=dev), torch.full((B * 64,), float("nan"), device=dev)
        if r1:
            lib.wm_relu_bwd_reduce_mask_r1(p(g1), p(hw), p(f["mask"]), p(f["y2"]), p(part), p(dzm), B, T, st())
        else:
            lib.wm_relu_bwd_reduce_mask(p(frame), p(f["mask"]), p(f["y2"]), None, p(part), p(dzm), B, T, st())
        res.append((part, dzm))
    eq(res[1][0], res[0][0], "partial")
    eq(res[1][1], res[0][1], "dzmax")
    assert bool(torch.isfinite(res[0][0]).all()) and float(res[0][1].max()) > 0
    # dzmax == NULL is allowed, as in the frame entry point
    part = torch.full((B * 128,), float("nan"), device=dev)
    lib.wm_relu_bwd_reduce_mask_r1(p(g1), p(hw), p(f["mask"]), p(f["y2"]), p(part), None, B, T, st())
    eq(part, res[0][0], "partial without dzmax")


# ------------------------------------------------------------------------------- 3. both fused convolution-backward launches
def _dwgrad(lib, r1, form, f, frame, g1, hw, k, gs, w, dzin, B, T, acc, dev):
    """one launch of the conv2 pair (form 2) / the conv1 pair (form 1) on the frame (r1 False) or on (g1, hw): every output"""
    from awm_amd import ops
    y = torch.full_like(f["x"], float("nan"))
    stats = torch.full((NCU * 128,), float("nan"), device=dev) if form == 2 else None
    wpart = torch.full((NCU * (3 * 4096 + 64),), float("nan"), device=dev)
    dw, db = rnd(64, 64, 3, seed=71).to(dev), rnd(64, seed=72).to(dev)          # what accumulate = 1 adds to
    dzmax = torch.full((NCU,), float("nan"), device=dev)
    wp = ops.pack_w64_h(w, 1)
    if form == 2:
        args = (p(None if r1 else frame), p(f["y2"]), p(k[0]), p(k[1]), p(k[3]), p(wp), p(f["y1"]), p(f["sc1"]), p(f["sh1"]),
                p(f["y1"]), p(f["sc1"]), p(f["sh1"]), p(y), p(stats), p(wpart), p(dw), p(db), B, T, 1, 1, acc, p(f["mask"]), 1, p(gs), p(dzmax))
    else:
        args = (p(dzin), p(f["y1"]), p(k[0]), p(k[1]), p(k[3]), p(wp), p(f["x"]), None, None,
                p(None if r1 else frame), None, None, p(y), None, p(wpart), p(dw), p(db), B, T, 0, 2, acc, p(f["mask"]), 1, p(gs), p(dzmax))
    if r1:
        lib.wm_dwgrad64_bf_r1(*args, p(g1), p(hw), st())
    else:
        lib.wm_dwgrad64_bf(*args, st())
    return dict(y=y, stats=stats, dw=dw, db=db, dzmax=dzmax)


def _compare(got, ref, what):
    for k_, v in ref.items():
        if v is not None:
            eq(got[k_], v, f"{what} {k_}")
    assert bool(torch.isfinite(ref["y"]).all()) and bool(torch.isfinite(ref["dw"]).all())


# (2, 64): one tile per clip, both halos outside the clip; (3, 192): interior tiles with real halos on both sides; (5, 8192): 640
# tiles on 256 workgroups, a workgroup walks three tiles (the tile + 2 tstep refills and the fetched-ahead epilogue operand are
# live); (1, 128): grid < 256, the stats / dzmax memset path
@pytest.mark.parametrize("B,T", [(2, 64), (3, 192), (5, 8192), (1, 128)])
@pytest.mark.parametrize("scale", SCALES)
def test_dwgrad64_bf_r1_both_pairs(awm, dev, B, T, scale):
    lib = awm.lib
    f = block_frames(lib, B, T, dev)
    g1, hw = upstream(B, T, scale, dev)
    frame, _, _ = head1_bwd(lib, g1, f["out"], hw, True)
    n = float(B * T)
    part, dzm = torch.empty(B * 128, device=dev), torch.empty(B * 64, device=dev)
    lib.wm_relu_bwd_reduce_mask(p(frame), p(f["mask"]), p(f["y2"]), None, p(part), p(dzm), B, T, st())
    k2, gs2 = finalize(lib, part, B, n, bn_stats(dev, 51), dzm, B * 64, dev)
    w2, w1 = rnd(64, 64, 3, seed=61, scale=0.1).to(dev), rnd(64, 64, 3, seed=62, scale=0.1).to(dev)
    ref2 = None
    for acc in (0, 1):
        ref2 = _dwgrad(lib, False, 2, f, frame, g1, hw, k2, gs2, w2, None, B, T, acc, dev)
        got2 = _dwgrad(lib, True, 2, f, frame, g1, hw, k2, gs2, w2, None, B, T, acc, dev)
        _compare(got2, ref2, f"conv2 pair accumulate={acc}")
    assert float(ref2["y"].abs().max()) > 0
    k1, gs1 = finalize(lib, ref2["stats"], NCU, n, bn_stats(dev, 54), ref2["dzmax"], NCU, dev)
    for acc in (0, 1):
        ref1 = _dwgrad(lib, False, 1, f, frame, g1, hw, k1, gs1, w1, ref2["y"], B, T, acc, dev)
        got1 = _dwgrad(lib, True, 1, f, frame, g1, hw, k1, gs1, w1, ref2["y"], B, T, acc, dev)
        _compare(got1, ref1, f"conv1 pair accumulate={acc}")


# ------------------------------------------------------------------------------- 4. invalid arguments
def test_invalid_arguments_launch_nothing(awm, dev):
    from awm_amd import ops
    lib = awm.lib
    B, T = 2, 64
    f = block_frames(lib, B, T, dev)
    g1, hw = upstream(B, T, 1.0, dev)
    k, gs = torch.ones(4, 64, device=dev), torch.ones(2, device=dev)
    wp = ops.pack_w64_h(rnd(64, 64, 3, seed=61, scale=0.1).to(dev), 1)
    torch.cuda.synchronize()

    def call(T_=T, g1_=g1, epi=1, xpro=1, gmask=f["mask"], arith=1, g=None, hw_=hw):
        y, stats = torch.full_like(f["x"], 7.0), torch.full((NCU * 128,), 7.0, device=dev)
        wpart, dw, db, dzmax = (torch.full((m,), 7.0, device=dev) for m in (NCU * (3 * 4096 + 64), 64 * 64 * 3, 64, NCU))
        with pytest.raises(RuntimeError, match=f"hipError {INVALID}$"):
            lib.wm_dwgrad64_bf_r1(p(g), p(f["y2"]), p(k[0]), p(k[1]), p(k[3]), p(wp), p(f["y1"]), p(f["sc1"]), p(f["sh1"]),
                                  p(f["y1"]), p(f["sc1"]), p(f["sh1"]), p(y), p(stats), p(wpart), p(dw), p(db), B, T_, xpro, epi, 0,
                                  p(gmask), arith, p(gs), p(dzmax), p(g1_), p(hw_), st())
        torch.cuda.synchronize()
        for t in (y, stats, wpart, dw, db, dzmax):
            assert bool((t == 7.0).all()), "an invalid call must launch nothing"
    call(g1_=None)                   # no row
    call(hw_=None)                   # no weights
    call(T_=96)                      # T % 64 != 0
    call(epi=8, xpro=0)              # the folded conv1 pair has no rank-one build
    call(epi=1, xpro=0)              # a pairing that does not exist
    call(gmask=None)                 # the rank-one builds mask on load
    call(arith=0)                    # bf16x6 keeps the materialised frame
    call(g=f["x"])                   # conv2 pair: the frame stands in for g, which must be null
    part, dzm = torch.full((B * 128,), 7.0, device=dev), torch.full((B * 64,), 7.0, device=dev)
    for a in ((None, p(hw), p(f["mask"]), 64), (p(g1), None, p(f["mask"]), 64), (p(g1), p(hw), None, 64), (p(g1), p(hw), p(f["mask"]), 62)):
        with pytest.raises(RuntimeError, match=f"hipError {INVALID}$"):
            lib.wm_relu_bwd_reduce_mask_r1(a[0], a[1], a[2], p(f["y2"]), p(part), p(dzm), B, a[3], st())
    torch.cuda.synchronize()
    assert bool((part == 7.0).all()) and bool((dzm == 7.0).all())


# ------------------------------------------------------------------------------- 5. the tape node
SPIED = ("wm_head1_bwd", "wm_relu_bwd_reduce_mask", "wm_relu_bwd_reduce_mask_r1", "wm_dwgrad64_bf", "wm_dwgrad64_bf_r1")
TODAY = (1, 1, 0, 2, 0)            # calls of SPIED on the route of today
RANK1 = (1, 0, 1, 0, 2)


@pytest.fixture(scope="module")
def gen(awm, dev):
    G, _ = reference_models(awm, dev)
    return G.train()


def _node(awm, gen, dev, on, monkeypatch, B, T):
    """decoder.1 -> decoder.2 as ops.ResBlockHead1Fn, forward and backward, on a copy of the Generator:
    ({name: gradient}, calls of SPIED, the dx arguments wm_head1_bwd saw)"""
    from awm_amd import ops
    from awm_amd.modules import _rb_args
    G = copy.deepcopy(gen)
    rb, head = G.decoder[1], G.decoder[2]
    x = rnd(B, 64, T, seed=81).to(dev).requires_grad_()
    up = rnd(B, 1, T, seed=82)
    up[:, :, ::7] = 0.0
    dxs = []
    before = ops._HEAD1_R1["on"]
    ops.set_head1_rank1(on)
    try:
        with monkeypatch.context() as mp:
            real = awm.lib.wm_head1_bwd
            mp.setattr(awm.lib, "wm_head1_bwd", lambda *a: (dxs.append(a[3]), real(*a))[1])
            counts = _spy(mp, awm.lib, SPIED)
            y = ops.ResBlockHead1Fn.apply(x, *_rb_args(rb), head.weight, head.bias)
            y.backward(up.to(dev))
            ops.join_side_stream()
    finally:
        ops.set_head1_rank1(before)
    torch.cuda.synchronize()
    grads = {k: q.grad for k, q in G.named_parameters() if q.grad is not None}
    grads["x"] = x.grad
    return grads, tuple(counts.get(n, 0) for n in SPIED), dxs


def _equal(a, b):
    assert set(a) == set(b) and "x" in a and "decoder.2.weight" in a and "decoder.1.block.0.weight" in a
    for k in b:
        assert torch.equal(bits(a[k]), bits(b[k])), f"gradient {k}"
        assert bool(torch.isfinite(b[k]).all())


@pytest.mark.parametrize("B,T", [(3, 192), (2, 8192)])
def test_tape_node_switch_on_against_off(awm, dev, gen, monkeypatch, B, T):
    on, con, dx_on = _node(awm, gen, dev, True, monkeypatch, B, T)
    off, coff, dx_off = _node(awm, gen, dev, False, monkeypatch, B, T)
    assert con == RANK1 and dx_on == [None], "switch on: no frame is written, no reader of a frame runs"
    assert coff == TODAY and len(dx_off) == 1 and dx_off[0] is not None, "switch off: the sequence of today"
    _equal(on, off)


@pytest.mark.parametrize("what", ["T % 64 != 0", "bwd_f16x3 off", "side-stream weight gradients"])
def test_tape_node_fallbacks_take_the_route_of_today(awm, dev, gen, monkeypatch, what):
    from awm_amd import ops
    B, T = 2, 192
    want = TODAY
    if what == "T % 64 != 0":
        T, want = 200, (1, 1, 0, 0, 0)        # (the unfused ResBlock backward: no wm_dwgrad64_bf at all)
    if what == "side-stream weight gradients":
        monkeypatch.setitem(ops._ASYNC, "on", True)
    with ops.switches(bwd_f16x3=(what != "bwd_f16x3 off")):
        on, con, dx_on = _node(awm, gen, dev, True, monkeypatch, B, T)
        off, coff, _ = _node(awm, gen, dev, False, monkeypatch, B, T)
    assert con == coff == want and dx_on[0] is not None
    _equal(on, off)


# ------------------------------------------------------------------------------- 6. one whole train step of main16
# T: a whole step needs T > 1024 (the loudness STFT reflect-pads by 1024 steps: wm_loud_loss rejects T <= 1024 on either route), and
# the default routes of the other nodes (tail in consumer) need T % 128 == 0: 1152 is the smallest such clip.
def test_train_step_switch_on_against_off(awm, dev, monkeypatch):
    from awm_amd import ops
    B, T = 2, 1152
    G0, D0 = reference_models(awm, dev)
    s = O.synthetic_clips(B, seed=91, T=T).to(dev)
    msg = O.synthetic_messages(B, seed=92, bits=16).to(dev)
    res = []
    before = ops._HEAD1_R1["on"]
    try:
        for on in (True, False):
            ops.set_head1_rank1(on)
            G, D = copy.deepcopy(G0).train(), copy.deepcopy(D0).train()
            opt = torch.optim.Adam(list(G.parameters()) + list(D.parameters()), lr=1e-3)
            with monkeypatch.context() as mp:
                counts = _spy(mp, awm.lib, SPIED)
                out = awm.train_step(G, D, opt, s, msg)
            torch.cuda.synchronize()
            res.append(dict(out={k: v.detach() for k, v in out.items() if isinstance(v, torch.Tensor)},
                            grads={f"{n}.{k}": q.grad for n, m in (("G", G), ("D", D)) for k, q in m.named_parameters()},
                            state={f"{n}.{k}": v for n, m in (("G", G), ("D", D)) for k, v in m.state_dict().items()},
                            counts=tuple(counts.get(n, 0) for n in SPIED)))
    finally:
        ops.set_head1_rank1(before)
    on, off = res
    # decoder.1 is the one block behind a rank-one head; the other five blocks keep wm_dwgrad64_bf
    assert on["counts"][2] == 1 and on["counts"][4] == 2 and off["counts"][2] == 0 and off["counts"][4] == 0
    assert on["counts"][3] + 2 == off["counts"][3] and on["counts"][1] + 1 == off["counts"][1]
    assert "total" in on["out"] and bool(torch.isfinite(on["out"]["total"]))
    for part in ("out", "grads", "state"):
        assert set(on[part]) == set(off[part])
        for k in off[part]:
            assert same(on[part][k], off[part][k]), f"{part} {k}: differs between the routes"
    assert all(v is not None for v in off["grads"].values())
