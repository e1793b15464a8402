"""The ResBlock tail and both BCE terms inside the head kernels (wm_headN_tail_fwd, wm_head1_tail_fwd, wm_headN_bwd_bce) against the
launches they replace (wm_bn_add_relu_mask + wm_headN_fwd / wm_head1_fwd, wm_bce_fwd, wm_bce_bwd + wm_headN_bwd), and the two tape
nodes built on them against the switch-off route.  Everything except the two loss sums must agree bit for bit; the sums are held to
fp64 on the same logits, at most twice as far from it as wm_bce_fwd is (plus one fp32 ulp of the sum: the final rounding to float
is up to half an ulp for either grouping, whatever came before it)."""
import copy

import pytest
import torch
import torch.nn.functional as F

from gpu_support import awm, dev  # noqa: F401
from gpu_support import _spy, p, rnd, st
from oracle import wm_oracle as O

pytestmark = pytest.mark.gpu

# (R rows, B labelled rows, T): 64 = one full wave; 200 = a partial last wave and a partial last mask word (200 % 32 = 8);
# 320 = two tiles, the second partial; 36 = less than a wave
SHAPES = [(4, 2, 64), (4, 2, 200), (4, 2, 320), (3, 1, 36)]
WIDTHS = [1, 17, 9, 33]          # both exact-width builds, and the run-time width below and above 32
FP32_ULP = 2.0 ** -23


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def frames(R, T, dev):
    """x, y2, scale, shift such that out = relu(x + y2*scale + shift) has both signs in front of the ReLU and exact zeros that are
    not clamped negatives (channel 5: shift 0 and x = y2 = 0 at every 7th step)"""
    x, y2 = rnd(R, 64, T, seed=11 + T), rnd(R, 64, T, seed=12 + T)
    sc, sh = rnd(64, seed=13).abs() + 0.5, rnd(64, seed=14, scale=0.3)
    sh[5] = 0.0
    x[:, 5, ::7] = 0.0
    y2[:, 5, ::7] = 0.0
    return x.to(dev), y2.to(dev), sc.to(dev), sh.to(dev)


def head_params(NO, dev, scale=1.0):
    return (rnd(NO, 64, 1, seed=21 + NO, scale=0.2) * scale).to(dev), (rnd(NO, seed=22 + NO, scale=0.1) * scale).to(dev)


def two_launch_tail(lib, x, y2, sc, sh):
    R, _, T = x.shape
    out = torch.empty_like(x)
    mask = torch.full((R * 64 * ((T + 31) // 32),), -1, dtype=torch.int32, device=x.device)
    lib.wm_bn_add_relu_mask(p(x), p(y2), p(sc), p(sh), p(out), p(mask), R, T, st())
    return out, mask


def messages(B, NO, kind, dev):
    if NO == 1 or kind == "zeros":
        m = torch.zeros(B, dtype=torch.int64)
    elif kind == "ones":
        m = torch.full((B,), (1 << (NO - 1)) - 1, dtype=torch.int64)
    else:
        m = torch.randint(0, 1 << (NO - 1), (B,), generator=torch.Generator().manual_seed(31 + NO), dtype=torch.int64)
    return m.to(dev)


def fp64_losses(logits, msg, B):
    """(loc, bce) of py/main16.py:252-264 in fp64 on the given logits [R,T,NO]; bce None at NO == 1"""
    lg = logits.double()
    R, T, NO = lg.shape
    label = torch.zeros(R, T, dtype=torch.float64, device=lg.device)
    label[:B] = 1.0
    loc = F.binary_cross_entropy_with_logits(lg[:, :, 0], label)
    if NO == 1:
        return float(loc), None
    bit = ((msg[:, None] >> torch.arange(NO - 1, device=lg.device)) & 1).double()[:, None, :].expand(B, T, NO - 1)
    return float(loc), float(F.binary_cross_entropy_with_logits(lg[:B, :, 1:], bit))


# ------------------------------------------------------------------------------- 1. tail + head forward, through the C ABI
@pytest.mark.parametrize("R,B,T", SHAPES)
@pytest.mark.parametrize("NO", WIDTHS)
def test_headN_tail_fwd_matches_two_launches(awm, dev, NO, R, B, T):
    lib = awm.lib
    x, y2, sc, sh = frames(R, T, dev)
    w, b = head_params(NO, dev)
    out_ref, mask_ref = two_launch_tail(lib, x, y2, sc, sh)
    assert bool((out_ref == 0).any()) and bool((out_ref > 0).any()) and bool(((x + y2 * sc[None, :, None] + sh[None, :, None]) < 0).any())
    lg_ref = torch.empty(R, T, NO, device=dev)
    lib.wm_headN_fwd(p(out_ref), p(w), p(b), p(lg_ref), R, T, NO, st())
    out = torch.full_like(x, float("nan"))
    mask = torch.full_like(mask_ref, 0x55555555)          # every word must be written, the bits past T as zeros
    lg = torch.full_like(lg_ref, float("nan"))
    lib.wm_headN_tail_fwd(p(x), p(y2), p(sc), p(sh), p(w), p(b), None, 0, None, None, None, p(out), p(mask), p(lg), R, T, NO, st())
    assert bits_equal(out, out_ref), "out"
    assert torch.equal(mask, mask_ref), "mask words"
    assert bits_equal(lg, lg_ref), "logits"
    if T % 32:
        last = mask.view(R * 64, -1)[:, -1]
        assert int((last >> (T % 32)).abs().max()) == 0, "bits past T must be zero"
    # mask == NULL (training mode without gradients): same out and logits
    out2, lg2 = torch.full_like(x, float("nan")), torch.full_like(lg_ref, float("nan"))
    lib.wm_headN_tail_fwd(p(x), p(y2), p(sc), p(sh), p(w), p(b), None, 0, None, None, None, p(out2), None, p(lg2), R, T, NO, st())
    assert bits_equal(out2, out_ref) and bits_equal(lg2, lg_ref)
    # y2 == NULL: no tail, the plain head on x
    lg3, lg3_ref = torch.full_like(lg_ref, float("nan")), torch.empty_like(lg_ref)
    lib.wm_headN_fwd(p(x), p(w), p(b), p(lg3_ref), R, T, NO, st())
    lib.wm_headN_tail_fwd(p(x), None, None, None, p(w), p(b), None, 0, None, None, None, None, None, p(lg3), R, T, NO, st())
    assert bits_equal(lg3, lg3_ref)


@pytest.mark.parametrize("R,B,T", SHAPES)
def test_head1_tail_fwd_matches_two_launches(awm, dev, R, B, T):
    lib = awm.lib
    x, y2, sc, sh = frames(R, T, dev)
    w, b = head_params(1, dev)
    out_ref, mask_ref = two_launch_tail(lib, x, y2, sc, sh)
    y_ref = torch.empty(R, 1, T, device=dev)
    lib.wm_head1_fwd(p(out_ref), p(w), p(b), p(y_ref), R, T, st())
    for with_mask in (True, False):
        out, y = torch.full_like(x, float("nan")), torch.full_like(y_ref, float("nan"))
        mask = torch.full_like(mask_ref, 0x55555555) if with_mask else None
        lib.wm_head1_tail_fwd(p(x), p(y2), p(sc), p(sh), p(w), p(b), p(out), p(mask), p(y), R, T, st())
        assert bits_equal(out, out_ref), "out"
        assert bits_equal(y, y_ref), "delta_raw"
        if with_mask:
            assert torch.equal(mask, mask_ref), "mask words"


# ------------------------------------------------------------------------------- 2. the two BCE sums
@pytest.mark.parametrize("R,B,T", SHAPES)
@pytest.mark.parametrize("NO", WIDTHS)
def test_bce_sums_in_head_forward(awm, dev, NO, R, B, T):
    lib = awm.lib
    x, y2, sc, sh = frames(R, T, dev)
    nblk = R * ((T + 255) // 256)
    for gain in (1.0, 10.0, 40.0):       # 40: softplus in its series branch and near saturation
        w, b = head_params(NO, dev, scale=gain)
        for kind in ("zeros", "ones", "mixed"):
            msg = messages(B, NO, kind, dev)
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
            loc64, bce64 = fp64_losses(lg, msg, B)
            what = f"NO={NO} gain={gain} {kind}"
            e_f, e_u = abs(float(res[0]) - loc64), abs(float(un[0]) - loc64)
            print(f"{what}: loc {loc64:.9g} fused err {e_f:.3e} unfused err {e_u:.3e}")
            assert e_f <= 2.0 * e_u + FP32_ULP * abs(loc64), f"loc {what}: {e_f:.3e} vs unfused {e_u:.3e}"
            if NO == 1:
                assert float(res[1]) == 123.0, "NO == 1 must leave bce_out untouched"
            else:
                e_f, e_u = abs(float(res[1]) - bce64), abs(float(un[1]) - bce64)
                print(f"{what}: bce {bce64:.9g} fused err {e_f:.3e} unfused err {e_u:.3e}")
                assert e_f <= 2.0 * e_u + FP32_ULP * abs(bce64), f"bce {what}: {e_f:.3e} vs unfused {e_u:.3e}"
    # without the tail (a head behind an inference ResBlock): same sums from the same logits
    w, b = head_params(NO, dev)
    msg = messages(B, NO, "mixed", dev)
    out, _ = two_launch_tail(lib, x, y2, sc, sh)
    ra, rb = torch.full((2,), 123.0, device=dev), torch.full((2,), 123.0, device=dev)
    la, lb = torch.empty(R, T, NO, device=dev), torch.empty(R, T, NO, device=dev)
    pa, pb = torch.empty(2 * nblk, device=dev), torch.empty(2 * nblk, device=dev)
    lib.wm_headN_tail_fwd(p(x), p(y2), p(sc), p(sh), p(w), p(b), p(msg), B, p(pa), p(ra[0]), p(ra[1]), p(torch.empty_like(x)), None, p(la), R, T, NO, st())
    lib.wm_headN_tail_fwd(p(out), None, None, None, p(w), p(b), p(msg), B, p(pb), p(rb[0]), p(rb[1]), None, None, p(lb), R, T, NO, st())
    assert bits_equal(la, lb) and bits_equal(ra, rb)


# ------------------------------------------------------------------------------- 3. dlogits formed on load
@pytest.mark.parametrize("R,B,T", SHAPES)
@pytest.mark.parametrize("NO", WIDTHS)
def test_headN_bwd_bce_matches_two_launches(awm, dev, NO, R, B, T):
    lib = awm.lib
    x = rnd(R, 64, T, seed=41).to(dev)
    w, _ = head_params(NO, dev)
    logits = rnd(R, T, NO, seed=42, scale=3.0).to(dev)
    msg = messages(B, NO, "mixed", dev)
    for gl, gb in ((10.0, 1.0), (0.0, 1.0), (10.0, 0.0)):
        g_loc, g_bce = torch.tensor([gl], device=dev), torch.tensor([gb], device=dev)
        for acc in (0, 1):
            res = []
            for fused in (False, True):
                dx = torch.full_like(x, float("nan"))
                dw, db = rnd(NO, 64, 1, seed=43).to(dev), rnd(NO, seed=44).to(dev)      # what accumulate = 1 adds to
                part = torch.empty(256 * (NO * 64 + NO), device=dev)
                if fused:
                    lib.wm_headN_bwd_bce(p(logits), p(msg), p(g_loc), p(g_bce), p(x), p(w), p(dx), p(part), p(dw), p(db), B, R, T, NO, acc, st())
                else:
                    d = torch.empty_like(logits)
                    lib.wm_bce_bwd(p(logits), p(msg), p(g_loc), p(g_bce), p(d), B, R, T, NO, st())
                    lib.wm_headN_bwd(p(d), p(x), p(w), p(dx), p(part), p(dw), p(db), R, T, NO, acc, st())
                res.append((dx, dw, db))
            for a, c, nm in zip(res[0], res[1], ("dx", "dw", "db")):
                assert bits_equal(a, c), f"{nm} NO={NO} g=({gl},{gb}) accumulate={acc}"
            assert bool(torch.isfinite(res[1][0]).all())


# ------------------------------------------------------------------------------- 4. whole nets, switch on against off
# The smallest clip forward_losses accepts that is a multiple of 64 and not of 256 (the fused ResBlock backward runs, the last
# 256-step tile of the heads is partial): the loudness STFT's reflect padding needs T > 2048 / 2, so 17 * 64, not 3 * 64.
NET_B, NET_T = 2, 1088
# loc / bce between the routes: each fp32 partial sum is at most 26 roundings deep in either grouping (16-17 terms in the thread, 6
# wave-shuffle levels, 4 waves), i.e. within 13 ulp of its exact value; the fp64 finish adds one rounding to float.  The totals add
# them with the weights 10 and 1 to terms that are equal on both routes.
SUM_ULPS = 32
def _models(awm, dev, bits, seed=5):
    torch.manual_seed(seed)
    G, D = awm.Generator(bits), awm.Detector(bits)
    return G.to(dev).train(), D.to(dev).train()


SPIED = ("wm_bn_add_relu_mask", "wm_bn_add_relu", "wm_bce_fwd", "wm_bce_bwd", "wm_headN_tail_fwd", "wm_head1_tail_fwd",
         "wm_headN_bwd_bce", "wm_headN_fwd", "wm_head1_fwd", "wm_headN_bwd")


def _step(awm, dev, G0, D0, s, msg, on, monkeypatch, extra=None, grad=True, hook=None):
    """one forward_losses (+ backward + Adam update) on copies of the models under the given switch value"""
    from awm_amd import ops
    G, D = copy.deepcopy(G0), copy.deepcopy(D0)
    if hook is not None:
        hook(G, D)
    s = s.clone().requires_grad_(grad)
    before = ops._HEADS["tail_in_head"]
    ops.set_tail_in_head(on)
    try:
        with monkeypatch.context() as mp:
            counts = _spy(mp, awm.lib, SPIED)
            with torch.enable_grad() if grad else torch.no_grad():
                total, out = awm.forward_losses(G, D, s, msg)
                saved = _final_blocks(out) if grad else None
                if extra is not None:
                    total = total + (out["logits"] * extra).sum()
                if grad:
                    opt = torch.optim.Adam(list(G.parameters()) + list(D.parameters()), lr=1e-3)
                    total.backward()
                    opt.step()
    finally:
        ops.set_tail_in_head(before)
    grads = {f"{n}.{k}": q.grad for n, m in (("G", G), ("D", D)) for k, q in m.named_parameters()} if grad else {}
    state = {f"{n}.{k}": v for n, m in (("G", G), ("D", D)) for k, v in m.state_dict().items()}
    return dict(out=out, grads=grads, state=state, ds=s.grad, counts=counts, saved=saved)


def _final_blocks(out):
    """(out, mask) of decoder.1 and of model.2, from the tape: the fused nodes save the block's nine tensors, then `out`; on the
    unfused route the head node saves `out` and the ResBlock node behind it the mask (index 3 of its block's nine)"""
    res = []
    for key in ("delta_raw", "logits"):
        node = out[key].grad_fn
        sv = node.saved_tensors
        if type(node).__name__.startswith(("ResBlockHead1Fn", "DetectorTailFn")):
            blk = sv[:9] if key == "delta_raw" else sv[9:18]
            res.append((sv[9] if key == "delta_raw" else sv[18], blk[3]))
        else:
            prev = sv[0].grad_fn.saved_tensors
            res.append((sv[0], prev[3] if key == "delta_raw" else prev[12]))
    return res


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and torch.equal(a, b), f"{what}: differs between the routes"


@pytest.mark.parametrize("bits", [0, 16, 8])
def test_whole_nets_switch_on_against_off(awm, dev, bits, monkeypatch):
    B, T = NET_B, NET_T
    G0, D0 = _models(awm, dev, bits)
    s = O.synthetic_clips(B, seed=61, T=T).to(dev)
    msg = O.synthetic_messages(B, seed=62, bits=bits).to(dev) if bits else torch.zeros(B, dtype=torch.int64, device=dev)
    on = _step(awm, dev, G0, D0, s, msg, True, monkeypatch)
    off = _step(awm, dev, G0, D0, s, msg, False, monkeypatch)
    # launches: three ResBlocks keep their own tail (encoder.1, encoder.2, model.1), no separate BCE passes
    assert off["counts"].get("wm_bn_add_relu_mask") == 5 and off["counts"].get("wm_bce_fwd") == 1 and off["counts"].get("wm_bce_bwd") == 1
    assert on["counts"].get("wm_bn_add_relu_mask") == 3
    assert "wm_bce_fwd" not in on["counts"] and "wm_bce_bwd" not in on["counts"] and "wm_bn_add_relu" not in on["counts"]
    assert on["counts"].get("wm_headN_tail_fwd") == 1 and on["counts"].get("wm_head1_tail_fwd") == 1 and on["counts"].get("wm_headN_bwd_bce") == 1
    assert "wm_headN_tail_fwd" not in off["counts"] and "wm_headN_bwd_bce" not in off["counts"]
    for (o1, m1), (o2, m2), nm in zip(on["saved"], off["saved"], ("decoder.1", "model.2")):
        _same(o1, o2, f"{nm} out")
        _same(m1, m2, f"{nm} mask")
    for k in ("delta_raw", "delta", "s_w", "logits", "l1", "mel", "loud", "hf"):
        _same(on["out"][k], off["out"][k], k)
    for k in off["grads"]:
        _same(on["grads"][k], off["grads"][k], f"grad {k}")
    _same(on["ds"], off["ds"], "ds")
    for k in off["state"]:
        _same(on["state"][k], off["state"][k], f"state after the update: {k}")
    # the two sums are grouped differently: rounding only (SUM_ULPS); the totals carry them
    for k in ("loc", "bce", "raw_total", "total"):
        a, b = float(on["out"][k]), float(off["out"][k])
        assert abs(a - b) <= SUM_ULPS * FP32_ULP * max(abs(b), 1.0), f"{k}: {a!r} vs {b!r}"
    lg = on["out"]["logits"].detach()
    loc64, bce64 = fp64_losses(lg, msg, B)
    for k, ref in (("loc", loc64), ("bce", bce64)):
        if ref is not None:
            e_f, e_u = abs(float(on["out"][k]) - ref), abs(float(off["out"][k]) - ref)
            assert e_f <= 2.0 * e_u + FP32_ULP * abs(ref), f"{k}: fused {e_f:.3e} unfused {e_u:.3e} from fp64"


# ------------------------------------------------------------------------------- 5. fallbacks
def test_forward_hook_takes_the_unfused_route(awm, dev, monkeypatch):
    B, T = NET_B, NET_T
    G0, D0 = _models(awm, dev, 16)
    s = O.synthetic_clips(B, seed=63, T=T).to(dev)
    msg = O.synthetic_messages(B, seed=64, bits=16).to(dev)

    def hook(G, D):
        D.model[3].register_forward_hook(lambda m, i, o: None)
        G.decoder[2].register_forward_hook(lambda m, i, o: None)
    on = _step(awm, dev, G0, D0, s, msg, True, monkeypatch, hook=hook)
    off = _step(awm, dev, G0, D0, s, msg, False, monkeypatch, hook=hook)
    assert "wm_headN_tail_fwd" not in on["counts"] and "wm_head1_tail_fwd" not in on["counts"] and on["counts"] == off["counts"]
    for k in ("delta_raw", "logits", "loc", "bce", "total"):
        _same(on["out"][k], off["out"][k], k)
    for k in off["grads"]:
        _same(on["grads"][k], off["grads"][k], f"grad {k}")


def test_gradient_fed_into_logits(awm, dev, monkeypatch):
    B, T = NET_B, NET_T
    G0, D0 = _models(awm, dev, 16)
    s = O.synthetic_clips(B, seed=65, T=T).to(dev)
    msg = O.synthetic_messages(B, seed=66, bits=16).to(dev)
    extra = rnd(2 * B, T, 17, seed=67, scale=1e-3).to(dev)
    on = _step(awm, dev, G0, D0, s, msg, True, monkeypatch, extra=extra)
    off = _step(awm, dev, G0, D0, s, msg, False, monkeypatch, extra=extra)
    assert on["counts"].get("wm_headN_tail_fwd") == 1 and on["counts"].get("wm_bce_bwd") == 1 and "wm_headN_bwd_bce" not in on["counts"]
    for k in off["grads"]:
        _same(on["grads"][k], off["grads"][k], f"grad {k}")
    _same(on["ds"], off["ds"], "ds")


def test_no_grad_in_training_mode(awm, dev, monkeypatch):
    B, T = NET_B, NET_T
    G0, D0 = _models(awm, dev, 16)
    s = O.synthetic_clips(B, seed=68, T=T).to(dev)
    msg = O.synthetic_messages(B, seed=69, bits=16).to(dev)
    on = _step(awm, dev, G0, D0, s, msg, True, monkeypatch, grad=False)
    off = _step(awm, dev, G0, D0, s, msg, False, monkeypatch, grad=False)
    for k in ("delta_raw", "delta", "logits", "l1", "mel", "loud", "hf"):
        _same(on["out"][k], off["out"][k], k)
    for k in off["state"]:
        _same(on["state"][k], off["state"][k], f"running statistics: {k}")
    for k in ("loc", "bce", "total"):
        a, b = float(on["out"][k]), float(off["out"][k])
        assert abs(a - b) <= SUM_ULPS * FP32_ULP * max(abs(b), 1.0), f"{k}: {a!r} vs {b!r}"
