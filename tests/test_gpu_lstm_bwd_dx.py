"""The LSTM input gradient formed on the helper waves of the wave-specialised BPTT launch (wm_lstm_bwd_wgrad_dx) against the two launches
it replaces (wm_lstm_bwd_wgrad, then wm_lstm_dx over the da tensor), and the route through ops.EncoderLSTMFn under
ops.set_lstm_dx_in_bwd.  The product is lstm_dx_bf_kernel's own -- the same fragments, pieces and product order, one accumulator chain
per tile -- and nothing else changes, so EVERYTHING must agree bit for bit."""
import copy

import pytest
import torch

from gpu_support import awm, dev  # noqa: F401
from gpu_support import _spy, p, reference_models, rnd, st

pytestmark = pytest.mark.gpu

NAN = float("nan")
SLAB = 256 * 128 + 256


def _lstm_params(dev):
    g = torch.Generator().manual_seed(181)
    wi, wh = (torch.rand(256, 64, generator=g) - 0.5) * 0.25, (torch.rand(256, 64, generator=g) - 0.5) * 0.25
    bi, bh = (torch.rand(256, generator=g) - 0.5) * 0.25, (torch.rand(256, generator=g) - 0.5) * 0.25
    return wi.to(dev), wh.to(dev), bi.to(dev), bh.to(dev)


_saved = {}


def _case(lib, dev, B, T):
    """inputs, parameters and wm_lstm_fwd_fused's saved tensors; computed once per shape and never written again"""
    if (B, T) not in _saved:
        wi, wh, bi, bh = _lstm_params(dev)
        x = rnd(B, 64, T, seed=182).to(dev)
        h, gates, cst = torch.empty_like(x), torch.empty(B, T, 256, device=dev), torch.empty(B, T, 64, device=dev)
        lib.wm_lstm_fwd_fused(p(x), p(wi), p(bi), p(bh), p(wh), p(h), p(gates), p(cst), B, T, st())
        _saved[(B, T)] = (x, h, gates, cst, wi, wh, rnd(B, 64, T, seed=183).to(dev))
    return _saved[(B, T)]


def _bases(dev):
    """what accumulate = 1 adds to"""
    return [rnd(*shape, seed=190 + i).to(dev) for i, shape in enumerate(((256, 64), (256, 64), (256,), (256,)))]


# ------------------------------------------------------------------------------- 1. the C ABI, bit for bit
# (1, 64) the minimum: one chunk's dx in the loop, one in the flush | (2, 96) an odd chunk count: both image buffers, the clip offset |
# (3, 160)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("scale", [1e-9, 1.0, 3e4])
@pytest.mark.parametrize("B,T", [(1, 64), (2, 96), (3, 160)])
def test_one_launch_matches_two(awm, dev, B, T, scale, accumulate):
    lib = awm.lib
    x, h, gates, cst, wi, wh, g = _case(lib, dev, B, T)
    dh = g * scale
    # the two launches, on a copy of gates (wm_lstm_bwd_wgrad leaves da there for wm_lstm_dx)
    ga, part_ref, dx_ref = gates.clone(), torch.full((B * SLAB,), NAN, device=dev), torch.full_like(x, NAN)
    dst_ref = _bases(dev)
    lib.wm_lstm_bwd_wgrad(p(ga), p(cst), p(dh), p(wh), p(x), p(h), p(part_ref), *map(p, dst_ref), B, T, accumulate, st())
    lib.wm_lstm_dx(p(ga), p(wi), p(dx_ref), B, T, st())
    assert bool(torch.isfinite(dx_ref).all()) and bool(torch.isfinite(part_ref).all()) and not torch.equal(ga, gates)
    # the one launch
    gb, part, dx = gates.clone(), torch.full((B * SLAB,), NAN, device=dev), torch.full_like(x, NAN)
    dst = _bases(dev)
    lib.wm_lstm_bwd_wgrad_dx(p(gb), p(cst), p(dh), p(wh), p(wi), p(x), p(h), p(part), *map(p, dst), p(dx), B, T, accumulate, st())
    assert torch.equal(dx, dx_ref), "dx"
    assert torch.equal(part, part_ref), "partial slabs"
    for name, a, r in zip(("dW_ih", "dW_hh", "db_ih", "db_hh"), dst, dst_ref):
        assert torch.equal(a, r), name
    assert torch.equal(gb, gates), "gates must keep the saved activations"


# ------------------------------------------------------------------------------- 2. rejections: an error, and nothing written
@pytest.mark.parametrize("B,T,null_dx", [(2, 48, False), (2, 32, False), (0, 64, False), (2, 64, True)],
                         ids=["T=48", "T=32", "B=0", "dx=NULL"])
def test_rejections(awm, dev, B, T, null_dx):
    lib = awm.lib
    nb = max(B, 1)
    wi, wh, _, _ = _lstm_params(dev)
    x, h, dh = rnd(nb, 64, T, seed=184).to(dev), rnd(nb, 64, T, seed=185).to(dev), rnd(nb, 64, T, seed=186).to(dev)
    gates, cst = torch.rand(nb, T, 256, device=dev), rnd(nb, T, 64, seed=187).to(dev)
    g0 = gates.clone()
    part, dx = torch.full((nb * SLAB,), NAN, device=dev), torch.full_like(x, NAN)
    dst = [torch.zeros(256, 64, device=dev), torch.zeros(256, 64, device=dev), torch.zeros(256, device=dev), torch.zeros(256, device=dev)]
    with pytest.raises(RuntimeError, match="wm_lstm_bwd_wgrad_dx"):
        lib.wm_lstm_bwd_wgrad_dx(p(gates), p(cst), p(dh), p(wh), p(wi), p(x), p(h), p(part), *map(p, dst),
                                 None if null_dx else p(dx), B, T, 0, st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(part).all()), "something was written"
    assert all(bool((t == 0).all()) for t in dst), "a gradient buffer was written"
    assert torch.equal(gates, g0)


# ------------------------------------------------------------------------------- 3. the route
ROUTE_B, ROUTE_T = 2, 128
SPIED = ("wm_lstm_bwd_wgrad_dx", "wm_lstm_bwd_wgrad", "wm_lstm_dx", "wm_lstm_bwd", "wm_lstm_bwd_fused", "wm_lstm_wgrad")


@pytest.fixture(scope="module")
def gen(awm, dev):
    G, _ = reference_models(awm, dev)
    return G.train()


def _run(awm, gen, dev, on, monkeypatch, node="encoder", T=ROUTE_T, flat=False):
    """encoder.1 -> encoder.2 -> LSTM and its backward on a copy of the Generator: ({name: gradient}, spied call counts).
    node = "encoder": ops.EncoderLSTMFn | "lstm": the two blocks as their pair node, then plain ops.LSTMFn.  flat: the LSTM's parameters
    carry side-stream gradient destinations (the caller has switched the option on)."""
    from awm_amd import ops
    from awm_amd.modules import _rb_args, resblock_pair
    G = copy.deepcopy(gen)
    e1, e2 = G.encoder[1], G.encoder[2]
    lstm = (G.lstm.weight_ih_l0, G.lstm.weight_hh_l0, G.lstm.bias_ih_l0, G.lstm.bias_hh_l0)
    if flat:
        for q in lstm:
            q._wm_grad = torch.zeros_like(q)
    x = rnd(ROUTE_B, 64, T, seed=188).to(dev).requires_grad_()
    before = ops._LSTM_DX["in_bwd"]
    ops.set_lstm_dx_in_bwd(on)
    try:
        with monkeypatch.context() as mp:
            counts = _spy(mp, awm.lib, SPIED)
            if node == "encoder":
                assert flat or ops.tail_in_consumer_applies(x, lstm=True)   # (the Generator never folds with the side stream on)
                y = ops.EncoderLSTMFn.apply(x, *_rb_args(e1), *_rb_args(e2), *lstm)
            else:
                y = ops.LSTMFn.apply(resblock_pair(e1, e2, x), *lstm)
            y.backward(rnd(ROUTE_B, 64, T, seed=189).to(dev))
            ops.join_side_stream()
    finally:
        ops.set_lstm_dx_in_bwd(before)
    torch.cuda.synchronize()
    grads = {k: q.grad for k, q in G.named_parameters() if q.grad is not None}
    grads["x"] = x.grad
    if flat:
        grads.update({f"flat{i}": q._wm_grad for i, q in enumerate(lstm)})
    return grads, tuple(counts.get(n, 0) for n in SPIED)


def _equal(a, b):
    assert set(a) == set(b) and "x" in a
    for k in b:
        assert torch.equal(a[k], b[k]), f"gradient {k}"


def test_encoder_lstm_node_switch_on_against_off(awm, dev, gen, monkeypatch):
    on, con = _run(awm, gen, dev, True, monkeypatch)
    off, coff = _run(awm, gen, dev, False, monkeypatch)
    assert con == (1, 0, 0, 0, 0, 0) and coff == (0, 1, 1, 0, 0, 0)
    assert "encoder.1.block.0.weight" in on and "lstm.bias_hh_l0" in on
    _equal(on, off)


def test_plain_lstm_node_keeps_the_two_launches(awm, dev, gen, monkeypatch):
    on, con = _run(awm, gen, dev, True, monkeypatch, node="lstm")
    off, coff = _run(awm, gen, dev, False, monkeypatch, node="lstm")
    assert con == coff == (0, 1, 1, 0, 0, 0)
    _equal(on, off)
    ref, _ = _run(awm, gen, dev, True, monkeypatch)
    _equal(ref, on)                                  # and the two nodes agree with each other


# what each fallback launches instead, as (wm_lstm_bwd_wgrad_dx, wm_lstm_bwd_wgrad, wm_lstm_dx, wm_lstm_bwd, wm_lstm_bwd_fused,
# wm_lstm_wgrad): never the new entry point.  Where the wave-specialised BPTT itself is off, "the two launches" are the older pairs.
@pytest.mark.parametrize("switches,want", [(dict(lstm_bwd_ws=False), (0, 0, 1, 1, 0, 1)),
                                           (dict(lstm_bwd_fused=True), (0, 0, 0, 0, 1, 1))], ids=["bwd_ws off", "bwd_fused on"])
def test_fallback_on_a_path_switch(awm, dev, gen, monkeypatch, switches, want):
    from awm_amd import ops
    with ops.switches(**switches):
        on, con = _run(awm, gen, dev, True, monkeypatch)
        off, coff = _run(awm, gen, dev, False, monkeypatch)
    assert con == coff == want
    _equal(on, off)


@pytest.mark.parametrize("T,want", [(96, (1, 0, 0, 0, 0, 0)), (48, (0, 0, 1, 1, 0, 1)), (32, (0, 0, 1, 1, 0, 1))])
def test_fallback_on_the_clip_length(awm, dev, monkeypatch, T, want):
    """_lstm_bwd itself (EncoderLSTMFn needs T % 128 == 0): T % 32 != 0 or T < 64 keeps the launches of today; 96 is eligible"""
    from awm_amd import ops
    wi, wh, bi, bh = _lstm_params(dev)
    x, dh = rnd(2, 64, T, seed=191).to(dev), rnd(2, 64, T, seed=192).to(dev)
    res = []
    for inside in (True, False):
        _, saved = ops._lstm_fwd(x, wi, wh, bi, bh, True)
        with monkeypatch.context() as mp:
            counts = _spy(mp, awm.lib, SPIED)
            res.append(ops._lstm_bwd(saved, (None,) * 4, dh, dx_inside=inside))
        if inside:
            assert tuple(counts.get(n, 0) for n in SPIED) == want
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_fallback_on_side_stream_weight_gradients(awm, dev, gen, monkeypatch):
    from awm_amd import ops
    monkeypatch.setitem(ops._ASYNC, "on", True)
    on, con = _run(awm, gen, dev, True, monkeypatch, flat=True)
    off, coff = _run(awm, gen, dev, False, monkeypatch, flat=True)
    assert con == coff == (0, 1, 1, 0, 0, 0)
    assert bool((on["flat0"] != 0).any()) and "lstm.weight_ih_l0" not in on
    _equal(on, off)


def test_native_fp32_dx_is_honoured_by_the_entry_point(awm, dev, gen, monkeypatch):
    """wm_set_lstm_dx_bf16x6(0) lives in the library, where ops cannot see it: ops still calls the new entry point, which then runs the
    two launches itself -- the same dx as the switch-off route under that setting"""
    lib = awm.lib
    lib.wm_set_lstm_dx_bf16x6(0, None)
    try:
        on, con = _run(awm, gen, dev, True, monkeypatch)
        off, coff = _run(awm, gen, dev, False, monkeypatch)
    finally:
        lib.wm_set_lstm_dx_bf16x6(1, None)
    assert con == (1, 0, 0, 0, 0, 0) and coff == (0, 1, 1, 0, 0, 0)
    _equal(on, off)
    bf, _ = _run(awm, gen, dev, True, monkeypatch)
    assert not torch.equal(bf["x"], on["x"]), "the setting changed nothing: the test did not reach the fp32 kernel"
