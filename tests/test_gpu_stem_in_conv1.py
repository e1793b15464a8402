"""The stem's output y0 = Conv1d(1, 64, 7, padding=3)(s) formed by the first ResBlock's conv1 launch while it stages its input
(wm_conv64_bf_stem) and by that block's conv1 pair in the backward (wm_dwgrad64_bf_stem), against the launches they replace
(wm_stem_fwd, then wm_conv64_bf / wm_dwgrad64_bf on the materialised frame), and the tape nodes built on them against the switch-off
route.  The formed element is stem_fwd_kernel's own fmaf chain and no sum is regrouped: EVERY comparison is bit for bit."""
import copy

import pytest
import torch

from gpu_support import awm, dev  # noqa: F401
from gpu_support import _spy, bits, p, reference_models, rnd, same, st
from oracle import wm_oracle as O

pytestmark = pytest.mark.gpu

NCU = 256
INVALID = 1                        # hipErrorInvalidValue
NAN = float("nan")


def eq(a, b, what):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), f"{what}: differs from the materialised-frame route"


# ------------------------------------------------------------------------------- inputs
def stem_params(dev, kind):
    """the stem's w [64,1,7] and bias [64]: "plain" | "dead channel" (channel 9: all-zero taps, bias -0.0: its output is a zero whose
    sign only the full chain keeps: -0.0 where all seven samples under the taps are negative, else +0.0) | "small" / "large" (scaled by
    1e-3 / 1e3)"""
    w, b = rnd(64, 1, 7, seed=31, scale=0.3), rnd(64, seed=32, scale=0.1)
    if kind == "dead channel":
        w[9] = 0.0
        b[9] = -0.0
    if kind == "small":
        w, b = w * 1e-3, b * 1e-3
    if kind == "large":
        w, b = w * 1e3, b * 1e3
    return w.to(dev), b.to(dev)


def clips(B, T, dev, kind):
    """s [B,1,T]: "synthetic" = the oracle's clips | "zero clip" = the same with one clip of exact zeros (the last one) | "negative
    run" = the same with samples 8..23 of every clip made negative (a signed-zero channel then shows both zeros)"""
    s = O.synthetic_clips(B, seed=33 + T, T=T)
    if kind == "zero clip":
        s[B - 1] = 0.0
    if kind == "negative run":
        s[:, :, 8:24] = -s[:, :, 8:24].abs() - 1e-3
    return s.to(dev)


CASES = [("synthetic", "plain"), ("zero clip", "plain"), ("negative run", "dead channel"), ("synthetic", "small"), ("synthetic", "large")]


def stem_fwd(lib, s, w, b):
    B, _, T = s.shape
    y0 = torch.full((B, 64, T), NAN, device=s.device)
    lib.wm_stem_fwd(p(s), p(w), p(b), p(y0), B, T, st())
    return y0


def conv_params(dev):
    from awm_amd import ops
    w, b = rnd(64, 64, 3, seed=71, scale=0.08).to(dev), rnd(64, seed=72, scale=0.1).to(dev)
    return ops.pack_w64_h(w, 0), b


# ------------------------------------------------------------------------------- 1. conv1 with the stem prologue, through the C ABI
# (1, 128) one tile, both halos outside the clip | (2, 256) an interior halo, and a halo across the clip boundary that must read zero,
# not the neighbour clip | (3, 384) | (5, 8192) 320 tiles on a grid of 256: more than one tile per workgroup
FWD_SHAPES = [(1, 128), (2, 256), (3, 384), (5, 8192)]


@pytest.mark.parametrize("B,T", FWD_SHAPES)
@pytest.mark.parametrize("clip_kind,stem_kind", CASES)
def test_conv1_stem_prologue_matches_two_launches(awm, dev, B, T, clip_kind, stem_kind):
    lib = awm.lib
    s = clips(B, T, dev, clip_kind)
    w, b = stem_params(dev, stem_kind)
    wph, bias = conv_params(dev)
    y0_ref = stem_fwd(lib, s, w, b)
    y_ref, stats_ref = torch.full_like(y0_ref, NAN), torch.full((NCU * 128,), NAN, device=dev)
    lib.wm_conv64_bf(p(y0_ref), None, p(wph), None, None, None, p(bias), None, None, None, p(y_ref), p(stats_ref), B, T, 0, 0, 1, st())
    assert bool(torch.isfinite(y0_ref).all()) and bool(torch.isfinite(y_ref).all()) and bool(torch.isfinite(stats_ref).all())
    assert (float(s[0].abs().max()) > 0 or (clip_kind == "zero clip" and B == 1)) and float(y_ref.abs().max()) > 0
    if stem_kind == "dead channel":
        dead = bits(y0_ref[:, 9])
        assert bool((y0_ref[:, 9] == 0).all()) and bool((dead == 0).any()) and bool((dead == -2 ** 31).any()), "the dead channel holds both zeros"
    y0, y, stats = torch.full_like(y0_ref, NAN), torch.full_like(y0_ref, NAN), torch.full_like(stats_ref, NAN)
    lib.wm_conv64_bf_stem(p(s), p(w), p(b), p(wph), p(bias), p(y0), p(y), p(stats), B, T, st())
    eq(y0, y0_ref, "y0")
    eq(y, y_ref, "y1")
    eq(stats, stats_ref, "stats partials")


# ------------------------------------------------------------------------------- 2. the conv1 pair with the stem-formed operand
SCALES = [1e-6, 1.0, 3e3]          # of the upstream gradient: max |dz| -> the f16 split's power-of-two scale moves with it
# (1, 128) grid < 256: the dzmax memset path, both halos outside the clip | (2, 256) interior halos and one across the clip boundary |
# (3, 192) an odd tile count per clip | (5, 8192) 640 tiles on 256 workgroups: the tile + 2 tstep refills are live
BWD_SHAPES = [(1, 128), (2, 256), (3, 192), (5, 8192)]


def _conv1_pair(lib, stem, B, T, dz1, y1, k, gs, wp, e1, acc, dev, s, w, b, y0):
    """one launch of the plain conv1 pair on the materialised y0 (stem False) or on (s, w, b): every output"""
    y = torch.full((B, 64, T), NAN, device=dev)
    wpart = torch.full((NCU * (3 * 4096 + 64),), NAN, device=dev)
    dw, db = rnd(64, 64, 3, seed=73).to(dev), rnd(64, seed=74).to(dev)          # what accumulate = 1 adds to
    dzmax = torch.full((NCU,), NAN, device=dev)
    if stem:
        lib.wm_dwgrad64_bf_stem(p(dz1), p(y1), p(k[0]), p(k[1]), p(k[3]), p(wp), p(e1), p(y), p(wpart), p(dw), p(db), B, T, acc,
                                p(gs), p(dzmax), p(s), p(w), p(b), st())
    else:
        lib.wm_dwgrad64_bf(p(dz1), p(y1), p(k[0]), p(k[1]), p(k[3]), p(wp), p(y0), None, None, p(e1), None, None, p(y), None, p(wpart),
                           p(dw), p(db), B, T, 0, 2, acc, None, 1, p(gs), p(dzmax), st())
    return dict(y=y, dw=dw, db=db, dzmax=dzmax)


def _bn_constants(lib, dz1, y1, B, T, dev):
    """k [4,64] = A, B hi, B lo, C and gscale [2] as wm_bn_bwd_finalize leaves them for a launch on dz1: sums and max |dz1| per clip"""
    part = torch.stack([dz1.sum(dim=2), (dz1 * y1).sum(dim=2)], dim=1).reshape(-1).contiguous()          # [B][2][64]
    dzm = dz1.abs().amax(dim=2).reshape(-1).contiguous()                                                # [B * 64]
    gamma, mu, inv = (rnd(64, seed=51).abs() + 0.5).to(dev), rnd(64, seed=52, scale=0.1).to(dev), (rnd(64, seed=53).abs() + 0.5).to(dev)
    k, gs = torch.empty(4, 64, device=dev), torch.empty(2, device=dev)
    dg, dbe = torch.empty(64, device=dev), torch.empty(64, device=dev)
    lib.wm_bn_bwd_finalize(p(part), B, float(B * T), p(gamma), p(mu), p(inv), p(k[0]), p(k[1]), p(k[3]), p(dg), p(dbe), 0, 0, p(dzm), B * 64,
                           p(gs), st())
    return k, gs


@pytest.mark.parametrize("B,T", BWD_SHAPES)
@pytest.mark.parametrize("scale", SCALES)
def test_conv1_pair_stem_operand_matches_the_materialised_frame(awm, dev, B, T, scale):
    from awm_amd import ops
    lib = awm.lib
    wp = ops.pack_w64_h(rnd(64, 64, 3, seed=62, scale=0.1).to(dev), 1)
    for clip_kind, stem_kind in (CASES if scale == 1.0 else CASES[:1]):
        s = clips(B, T, dev, clip_kind)
        w, b = stem_params(dev, stem_kind)
        y0 = stem_fwd(lib, s, w, b)
        dz1, y1, e1 = (rnd(B, 64, T, seed=81 + T) * scale).to(dev), rnd(B, 64, T, seed=82 + T).to(dev), (rnd(B, 64, T, seed=83 + T) * scale).to(dev)
        dz1[:, :, ::7] = 0.0
        k, gs = _bn_constants(lib, dz1, y1, B, T, dev)
        for acc in (0, 1):
            ref = _conv1_pair(lib, False, B, T, dz1, y1, k, gs, wp, e1, acc, dev, s, w, b, y0)
            got = _conv1_pair(lib, True, B, T, dz1, y1, k, gs, wp, e1, acc, dev, s, w, b, y0)
            for name, v in ref.items():
                assert bool(torch.isfinite(v).all()), name
                eq(got[name], v, f"{clip_kind}, {stem_kind}, accumulate={acc}: {name}")
            assert float(ref["dw"].abs().max()) > 0 and float(ref["y"].abs().max()) > 0 and float(ref["dzmax"].max()) > 0


# ------------------------------------------------------------------------------- 3. guards
def test_conv1_stem_prologue_guards(awm, dev):
    from awm_amd import ops
    lib = awm.lib
    B, T = 2, 256
    w, b = stem_params(dev, "plain")
    wph, bias = conv_params(dev)
    torch.cuda.synchronize()

    def call(T_=T, s_=True, w_=w, b_=b, wph_=wph, y0_=True, y_=True, stats_=True):
        s = clips(B, T_, dev, "synthetic")
        y0, y, stats = torch.full((B, 64, T_), 7.0, device=dev), torch.full((B, 64, T_), 7.0, device=dev), torch.full((NCU * 128,), 7.0, device=dev)
        with pytest.raises(RuntimeError, match=f"wm_conv64_bf_stem failed with hipError {INVALID}$"):
            lib.wm_conv64_bf_stem(p(s) if s_ else None, p(w_), p(b_), p(wph_), p(bias), p(y0) if y0_ else None, p(y) if y_ else None,
                                  p(stats) if stats_ else None, B, T_, st())
        torch.cuda.synchronize()
        for t in (y0, y, stats):
            assert bool((t == 7.0).all()), "an invalid call must write nothing"
    call(T_=200)                     # T % 128 != 0
    call(s_=False)
    call(w_=None)
    call(b_=None)
    call(wph_=None)
    call(y0_=False)
    call(y_=False)
    call(stats_=False)
    with ops.switches(schedule=0):   # the phase-serial kernel has no stem prologue
        call()


def test_conv1_pair_stem_operand_guards(awm, dev):
    from awm_amd import ops
    lib = awm.lib
    B, T = 2, 256
    w, b = stem_params(dev, "plain")
    wp = ops.pack_w64_h(rnd(64, 64, 3, seed=62, scale=0.1).to(dev), 1)
    k, gs = torch.ones(4, 64, device=dev), torch.ones(2, device=dev)
    torch.cuda.synchronize()

    def call(T_=T, null=None):
        s = clips(B, T_, dev, "synthetic")
        dz1, y1, e1 = (rnd(B, 64, T_, seed=84 + i).to(dev) for i in range(3))
        y = torch.full((B, 64, T_), 7.0, device=dev)
        wpart, dw, db, dzmax = (torch.full((m,), 7.0, device=dev) for m in (NCU * (3 * 4096 + 64), 64 * 64 * 3, 64, NCU))
        a = dict(g=dz1, g2=y1, ga=k[0], gb=k[1], gc=k[3], wpb=wp, e1=e1, y=y, partial=wpart, dw=dw, gscale=gs, s=s, stem_w=w, stem_b=b)
        if null is not None:
            a[null] = None
        with pytest.raises(RuntimeError, match=f"wm_dwgrad64_bf_stem failed with hipError {INVALID}$"):
            lib.wm_dwgrad64_bf_stem(p(a["g"]), p(a["g2"]), p(a["ga"]), p(a["gb"]), p(a["gc"]), p(a["wpb"]), p(a["e1"]), p(a["y"]),
                                    p(a["partial"]), p(a["dw"]), p(db), B, T_, 0, p(a["gscale"]), p(dzmax), p(a["s"]), p(a["stem_w"]),
                                    p(a["stem_b"]), st())
        torch.cuda.synchronize()
        for t in (y, wpart, dw, db, dzmax):
            assert bool((t == 7.0).all()), "an invalid call must write nothing"
    call(T_=200)                     # T % 64 != 0
    for name in ("g", "g2", "ga", "gb", "gc", "wpb", "e1", "y", "partial", "dw", "gscale", "s", "stem_w", "stem_b"):
        call(null=name)


# ------------------------------------------------------------------------------- 4. the tape nodes, switch on against off
# T: a whole step needs T > 1024 (the loudness STFT reflect-pads by 1024 steps), the routes need T % 128 == 0: 1152 is the smallest
NET_B, NET_T = 2, 1152
SPIED = ("wm_stem_fwd", "wm_conv64_bf_stem", "wm_dwgrad64_bf_stem", "wm_conv64_bf_tail", "wm_stem_bwd", "wm_dwgrad64_bf")
ON = (0, 2, 2, 2, 2)               # calls of SPIED[:5] per train step with the switch on
OFF = (2, 0, 0, 2, 2)


def _models(awm, dev, msg_bits):
    if msg_bits == 16:
        return reference_models(awm, dev)
    torch.manual_seed(7)
    G, D = awm.Generator(msg_bits).to(dev), awm.Detector(msg_bits).to(dev)
    return G, D


def _inputs(dev, msg_bits, T, seed):
    s = O.synthetic_clips(NET_B, seed=seed, T=T).to(dev)
    msg = O.synthetic_messages(NET_B, seed=seed + 1, bits=msg_bits).to(dev) if msg_bits else torch.zeros(NET_B, dtype=torch.int64, device=dev)
    return s, msg


def _switch(ops, on):
    before = ops._STEMC["on"]
    ops.set_stem_in_conv1(on)
    return before


def _train_step(awm, G0, D0, s, msg, on, monkeypatch, prepare=None):
    """one awm.train_step on copies of the models under the given switch value: outputs, gradients, the state after the Adam update"""
    from awm_amd import ops
    G, D = copy.deepcopy(G0).train(), copy.deepcopy(D0).train()
    if prepare is not None:
        prepare(G, D)
    opt = torch.optim.Adam(list(G.parameters()) + list(D.parameters()), lr=1e-3)
    before = _switch(ops, on)
    try:
        with monkeypatch.context() as mp:
            counts = _spy(mp, awm.lib, SPIED)
            out = awm.train_step(G, D, opt, s, msg)
    finally:
        ops.set_stem_in_conv1(before)
    torch.cuda.synchronize()
    return dict(out={k: v.detach() for k, v in out.items() if isinstance(v, torch.Tensor)},
                grads={f"{n}.{k}": q.grad for n, m in (("G", G), ("D", D)) for k, q in m.named_parameters()},
                state={f"{n}.{k}": v for n, m in (("G", G), ("D", D)) for k, v in m.state_dict().items()},
                counts=tuple(counts.get(n, 0) for n in SPIED))


def _all_same(on, off):
    assert "total" in on["out"] and bool(torch.isfinite(on["out"]["total"]))
    for part in ("out", "grads", "state"):
        assert set(on[part]) == set(off[part])
        for k in off[part]:
            assert same(on[part][k], off[part][k]), f"{part} {k}: differs between the routes"
    assert all(v is not None for v in off["grads"].values())


@pytest.mark.parametrize("msg_bits", [16, 0])
def test_train_step_switch_on_against_off(awm, dev, monkeypatch, msg_bits):
    G0, D0 = _models(awm, dev, msg_bits)
    s, msg = _inputs(dev, msg_bits, NET_T, 91)
    on = _train_step(awm, G0, D0, s, msg, True, monkeypatch)
    off = _train_step(awm, G0, D0, s, msg, False, monkeypatch)
    assert on["counts"][:5] == ON, "switch on: no stem launch, both first blocks form the stem's output in their conv1 launches"
    assert off["counts"][:5] == OFF, "switch off: the sequence of today"
    assert on["counts"][5] + 2 == off["counts"][5], "the two conv1 pairs behind a stem moved to wm_dwgrad64_bf_stem"
    _all_same(on, off)


def _nodes(awm, G0, D0, s, msg, on, monkeypatch, grad_rows):
    """Generator and Detector forward and backward outside the train step (Detector.forward: the pair node behind the stem), with an
    input gradient wanted on the clips: outputs, every gradient, ds"""
    from awm_amd import ops
    G, D = copy.deepcopy(G0).train(), copy.deepcopy(D0).train()
    sg, sd = s.clone().requires_grad_(), torch.cat([s, 0.5 * s], 0).requires_grad_()
    before = _switch(ops, on)
    try:
        with monkeypatch.context() as mp:
            counts = _spy(mp, awm.lib, SPIED)
            delta = G(sg, msg)
            logits = D(sd, input_grad_rows=grad_rows)
            (delta.square().sum() + logits.square().sum()).backward()
            ops.join_side_stream()
    finally:
        ops.set_stem_in_conv1(before)
    torch.cuda.synchronize()
    grads = {f"{n}.{k}": q.grad for n, m in (("G", G), ("D", D)) for k, q in m.named_parameters()}
    grads["sg"], grads["sd"] = sg.grad, sd.grad
    return dict(out=dict(delta=delta.detach(), logits=logits.detach()), grads=grads, counts=tuple(counts.get(n, 0) for n in SPIED))


@pytest.mark.parametrize("grad_rows", [None, NET_B])
def test_nodes_with_an_input_gradient_switch_on_against_off(awm, dev, monkeypatch, grad_rows):
    G0, D0 = _models(awm, dev, 16)
    s, msg = _inputs(dev, 16, 256, 93)
    on = _nodes(awm, G0, D0, s, msg, True, monkeypatch, grad_rows)
    off = _nodes(awm, G0, D0, s, msg, False, monkeypatch, grad_rows)
    assert on["counts"][:5] == ON and off["counts"][:5] == OFF
    for part in ("out", "grads"):
        assert set(on[part]) == set(off[part])
        for k in off[part]:
            assert off[part][k] is not None and same(on[part][k], off[part][k]), f"{part} {k}: differs between the routes"
    if grad_rows is not None:
        assert bool((off["grads"]["sd"][grad_rows:] == 0).all()) and bool((off["grads"]["sd"][:grad_rows] != 0).any()), "the clean half stays zero"


# ------------------------------------------------------------------------------- 5. fallbacks: the sequence of today, unchanged
@pytest.mark.parametrize("what", ["T % 128 != 0", "a forward hook on the stem", "WM_TAIL_IN_CONSUMER off"])
def test_fallbacks_take_the_route_of_today(awm, dev, monkeypatch, what):
    from awm_amd import ops
    G0, D0 = _models(awm, dev, 16)
    s, msg = _inputs(dev, 16, 1160 if what == "T % 128 != 0" else NET_T, 95)
    seen = []

    def prepare(G, D):
        if what == "a forward hook on the stem":
            G.encoder[0].register_forward_hook(lambda m, i, o: seen.append("G"))
            D.model[0].register_forward_hook(lambda m, i, o: seen.append("D"))
    tailc = ops._TAILC["on"]
    ops.set_tail_in_consumer(what != "WM_TAIL_IN_CONSUMER off")
    try:
        on = _train_step(awm, G0, D0, s, msg, True, monkeypatch, prepare=prepare)
        off = _train_step(awm, G0, D0, s, msg, False, monkeypatch, prepare=prepare)
    finally:
        ops.set_tail_in_consumer(tailc)
    assert on["counts"] == off["counts"] and on["counts"][:3] == (2, 0, 0)
    if what == "a forward hook on the stem":
        assert seen == ["G", "D"] * 2, "the hooks must fire on both routes"
    _all_same(on, off)


def test_eval_mode_takes_the_route_of_today(awm, dev, monkeypatch):
    from awm_amd import ops
    G0, D0 = _models(awm, dev, 16)
    s, msg = _inputs(dev, 16, NET_T, 97)
    res = []
    for on in (True, False):
        G, D = copy.deepcopy(G0).eval(), copy.deepcopy(D0).eval()
        before = _switch(ops, on)
        try:
            with monkeypatch.context() as mp:
                counts = _spy(mp, awm.lib, SPIED)
                out = awm.eval_forward(G, D, s, msg)
        finally:
            ops.set_stem_in_conv1(before)
        torch.cuda.synchronize()
        res.append((out, tuple(counts.get(n, 0) for n in SPIED)))
    assert res[0][1] == res[1][1] and res[0][1][1:3] == (0, 0) and res[0][1][0] >= 2
    assert same(dict(res[0][0]), dict(res[1][0]))
