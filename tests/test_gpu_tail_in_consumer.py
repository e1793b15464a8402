"""The ResBlock tail formed by the kernel that reads it next -- the next block's conv1 (wm_conv64_bf_tail) and the LSTM forward's helper
waves (wm_lstm_fwd_tail) -- against the launches they replace (wm_bn_add_relu_mask, then wm_conv64_bf / wm_lstm_fwd_fused), and the
tape nodes built on them against the switch-off route.  The fold is elementwise, in wm_bn_add_relu's own expression, and regroups no
sum: EVERYTHING must agree bit for bit, the loss sums included."""
import copy

import pytest
import torch

from gpu_support import awm, dev  # noqa: F401
from gpu_support import _spy, p, rnd, st
from oracle import wm_oracle as O
from test_gpu_tail_in_head import _models, _same, bits_equal, frames, two_launch_tail

pytestmark = pytest.mark.gpu

NAN = float("nan")
UNWRITTEN = 0x55555555          # what the mask is pre-filled with: a word that is not written shows up


def _mixed_signs(x, y2, sc, sh, out_ref):
    pre = x + y2 * sc[None, :, None] + sh[None, :, None]
    return bool((out_ref == 0).any()) and bool((out_ref > 0).any()) and bool((pre < 0).any())


# ------------------------------------------------------------------------------- 1. conv1 with the tail prologue, through the C ABI
# (1, 128) one tile, both halos out of range | (2, 256) a halo across a tile boundary and none across the clip boundary | (3, 384) |
# (12, 8192) 768 tiles, three per workgroup: the steady-state loop with the tile i + 2 prefetch
CONV_SHAPES = [(1, 128), (2, 256), (3, 384), (12, 8192)]


def _conv_params(awm, dev):
    from awm_amd import ops
    w, b = rnd(64, 64, 3, seed=71, scale=0.08).to(dev), rnd(64, seed=72, scale=0.1).to(dev)
    return ops.pack_w64_h(w, 0), b, ops.NCU


@pytest.mark.parametrize("B,T", CONV_SHAPES)
def test_conv1_tail_prologue_matches_two_launches(awm, dev, B, T):
    lib = awm.lib
    x, y2, sc, sh = frames(B, T, dev)
    wph, bias, ncu = _conv_params(awm, dev)
    out_ref, mask_ref = two_launch_tail(lib, x, y2, sc, sh)
    assert _mixed_signs(x, y2, sc, sh, out_ref)
    y_ref, stats_ref = torch.full_like(x, NAN), torch.full((ncu * 128,), NAN, device=dev)
    lib.wm_conv64_bf(p(out_ref), None, p(wph), None, None, None, p(bias), None, None, None, p(y_ref), p(stats_ref), B, T, 0, 0, 1, st())
    assert bool(torch.isfinite(y_ref).all()) and bool(torch.isfinite(stats_ref).all())
    for with_mask in (True, False):
        out, y, stats = torch.full_like(x, NAN), torch.full_like(x, NAN), torch.full_like(stats_ref, NAN)
        mask = torch.full_like(mask_ref, UNWRITTEN) if with_mask else None
        lib.wm_conv64_bf_tail(p(x), p(y2), p(wph), p(sc), p(sh), p(bias), p(out), p(mask), p(y), p(stats), B, T, st())
        assert bits_equal(out, out_ref), "out"
        assert bits_equal(y, y_ref), "y1"
        assert bits_equal(stats, stats_ref), "stats partials"
        if with_mask:
            assert torch.equal(mask, mask_ref), "mask words"


def test_conv1_tail_prologue_rejects_a_ragged_length(awm, dev):
    lib = awm.lib
    B, T = 2, 192
    x, y2, sc, sh = frames(B, T, dev)
    wph, bias, ncu = _conv_params(awm, dev)
    out, y, stats = torch.full_like(x, NAN), torch.full_like(x, NAN), torch.full((ncu * 128,), NAN, device=dev)
    mask = torch.full((B * 64 * (T // 32),), UNWRITTEN, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="wm_conv64_bf_tail"):
        lib.wm_conv64_bf_tail(p(x), p(y2), p(wph), p(sc), p(sh), p(bias), p(out), p(mask), p(y), p(stats), B, T, st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(y).all()) and bool(torch.isnan(stats).all()), "something was written"
    assert bool((mask == UNWRITTEN).all())


# ------------------------------------------------------------------------------- 2. LSTM forward with the tail in its helper waves
# (2, 64) the prologue chunk plus one steady-state chunk | (3, 160) an odd number of chunks | (2, 1024)
LSTM_SHAPES = [(2, 64), (3, 160), (2, 1024)]


def _lstm_params(dev):
    g = torch.Generator().manual_seed(81)
    wi, wh = (torch.rand(256, 64, generator=g) - 0.5) * 0.25, (torch.rand(256, 64, generator=g) - 0.5) * 0.25
    bi, bh = (torch.rand(256, generator=g) - 0.5) * 0.25, (torch.rand(256, generator=g) - 0.5) * 0.25
    return wi.to(dev), wh.to(dev), bi.to(dev), bh.to(dev)


@pytest.mark.parametrize("B,T", LSTM_SHAPES)
@pytest.mark.parametrize("save", [True, False])
def test_lstm_fwd_tail_matches_two_launches(awm, dev, B, T, save):
    lib = awm.lib
    x, y2, sc, sh = frames(B, T, dev)
    wi, wh, bi, bh = _lstm_params(dev)
    out_ref, mask_ref = two_launch_tail(lib, x, y2, sc, sh)
    assert _mixed_signs(x, y2, sc, sh, out_ref)

    def buffers():
        h = torch.full_like(x, NAN)
        gates = torch.full((B, T, 256), NAN, device=dev) if save else None
        cst = torch.full((B, T, 64), NAN, device=dev) if save else None
        return h, gates, cst
    h_ref, gates_ref, cst_ref = buffers()
    lib.wm_set_lstm_fwd_wave_specialised(1, None)
    lib.wm_lstm_fwd_fused(p(out_ref), p(wi), p(bi), p(bh), p(wh), p(h_ref), p(gates_ref), p(cst_ref), B, T, st())
    assert bool(torch.isfinite(h_ref).all())
    for with_mask in (True, False):
        h, gates, cst = buffers()
        out = torch.full_like(x, NAN)
        mask = torch.full_like(mask_ref, UNWRITTEN) if with_mask else None
        lib.wm_lstm_fwd_tail(p(x), p(y2), p(sc), p(sh), p(out), p(mask), p(wi), p(bi), p(bh), p(wh), p(h), p(gates), p(cst), B, T, st())
        assert bits_equal(out, out_ref), "out"
        assert bits_equal(h, h_ref), "h"
        if save:
            assert bits_equal(gates, gates_ref), "gates"
            assert bits_equal(cst, cst_ref), "cst"
        if with_mask:
            assert torch.equal(mask, mask_ref), "mask words"


def test_lstm_fwd_tail_rejects_a_ragged_length(awm, dev):
    """T % 32 != 0: the entry point documents an error and no write (the caller keeps the two launches)"""
    lib = awm.lib
    B, T = 2, 72
    x, y2, sc, sh = frames(B, T, dev)
    wi, wh, bi, bh = _lstm_params(dev)
    out, h = torch.full_like(x, NAN), torch.full_like(x, NAN)
    mask = torch.full((B * 64 * ((T + 31) // 32),), UNWRITTEN, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="wm_lstm_fwd_tail"):
        lib.wm_lstm_fwd_tail(p(x), p(y2), p(sc), p(sh), p(out), p(mask), p(wi), p(bi), p(bh), p(wh), p(h), None, None, B, T, st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(h).all()) and bool((mask == UNWRITTEN).all())


# ------------------------------------------------------------------------------- 3. whole nets, switch on against off
# the shortest clip forward_losses accepts (the loudness STFT's reflect padding needs T > 1024) that is a multiple of 128
NET_B, NET_T = 2, 2048
SPIED = ("wm_bn_add_relu_mask", "wm_bn_add_relu", "wm_conv64_bf_tail", "wm_lstm_fwd_tail", "wm_lstm_fwd_fused")


def _step(awm, G0, D0, s, msg, on, monkeypatch, grad=True, prepare=None):
    """one forward_losses (+ backward + Adam update) on copies of the models under the given switch value"""
    from awm_amd import ops
    G, D = copy.deepcopy(G0), copy.deepcopy(D0)
    if prepare is not None:
        prepare(G, D)
    s = s.clone().requires_grad_(grad)
    before = ops._TAILC["on"]
    ops.set_tail_in_consumer(on)
    try:
        with monkeypatch.context() as mp:
            counts = _spy(mp, awm.lib, SPIED)
            with torch.enable_grad() if grad else torch.no_grad():
                total, out = awm.forward_losses(G, D, s, msg)
                if grad:
                    opt = torch.optim.Adam(list(G.parameters()) + list(D.parameters()), lr=1e-3)
                    total.backward()
                    opt.step()
    finally:
        ops.set_tail_in_consumer(before)
    grads = {f"{n}.{k}": q.grad for n, m in (("G", G), ("D", D)) for k, q in m.named_parameters()} if grad else {}
    state = {f"{n}.{k}": v for n, m in (("G", G), ("D", D)) for k, v in m.state_dict().items()}
    return dict(total=total.detach(), out=out, grads=grads, state=state, ds=s.grad, counts=counts)


def _all_equal(on, off):
    _same(on["total"], off["total"], "total")
    assert set(on["out"]) == set(off["out"])
    for k, v in off["out"].items():
        if isinstance(v, torch.Tensor):
            _same(on["out"][k], v, f"out[{k}]")
        else:
            assert on["out"][k] == v, f"out[{k}]"
    assert set(on["grads"]) == set(off["grads"])
    for k in off["grads"]:
        _same(on["grads"][k], off["grads"][k], f"grad {k}")
    _same(on["ds"], off["ds"], "ds")
    for k in off["state"]:
        _same(on["state"][k], off["state"][k], f"state after the update: {k}")


def _inputs(dev, bits, T, seed):
    s = O.synthetic_clips(NET_B, seed=seed, T=T).to(dev)
    msg = O.synthetic_messages(NET_B, seed=seed + 1, bits=bits).to(dev) if bits else torch.zeros(NET_B, dtype=torch.int64, device=dev)
    return s, msg


def _count(r, name):
    return r["counts"].get(name, 0)


@pytest.mark.parametrize("bits", [16, 0])
def test_whole_nets_switch_on_against_off(awm, dev, bits, monkeypatch):
    G0, D0 = _models(awm, dev, bits)
    s, msg = _inputs(dev, bits, NET_T, 91)
    on = _step(awm, G0, D0, s, msg, True, monkeypatch)
    off = _step(awm, G0, D0, s, msg, False, monkeypatch)
    # encoder.1, encoder.2 and model.1 lose their tail launch (decoder.1's and model.2's already ride in the heads)
    assert (_count(on, "wm_bn_add_relu_mask"), _count(on, "wm_conv64_bf_tail"), _count(on, "wm_lstm_fwd_tail")) == (0, 2, 1)
    assert (_count(off, "wm_bn_add_relu_mask"), _count(off, "wm_conv64_bf_tail"), _count(off, "wm_lstm_fwd_tail")) == (3, 0, 0)
    assert _count(on, "wm_lstm_fwd_fused") == 0 and _count(off, "wm_lstm_fwd_fused") == 1 and _count(on, "wm_bn_add_relu") == 0
    _all_equal(on, off)


# ------------------------------------------------------------------------------- 4. fallbacks: the present route, unchanged
def test_ragged_length_takes_the_present_route(awm, dev, monkeypatch):
    G0, D0 = _models(awm, dev, 16)
    s, msg = _inputs(dev, 16, 1088, 93)                 # 17 * 64: the fused backward runs, the f16 pipelined forward does not
    on = _step(awm, G0, D0, s, msg, True, monkeypatch)
    off = _step(awm, G0, D0, s, msg, False, monkeypatch)
    assert on["counts"] == off["counts"] and _count(on, "wm_bn_add_relu_mask") == 3 and _count(on, "wm_conv64_bf_tail") == 0
    _all_equal(on, off)


@pytest.mark.parametrize("where", ["encoder.2", "lstm"])
def test_forward_hook_keeps_the_hooked_module_in_front_of_a_tensor(awm, dev, where, monkeypatch):
    G0, D0 = _models(awm, dev, 16)
    s, msg = _inputs(dev, 16, NET_T, 95)
    seen = []

    def prepare(G, D):
        (G.encoder[2] if where == "encoder.2" else G.lstm).register_forward_hook(lambda m, i, o: seen.append(where))
    on = _step(awm, G0, D0, s, msg, True, monkeypatch, prepare=prepare)
    off = _step(awm, G0, D0, s, msg, False, monkeypatch, prepare=prepare)
    assert _count(on, "wm_lstm_fwd_tail") == 0 and _count(on, "wm_lstm_fwd_fused") == 1, "the LSTM must read a materialised tensor"
    if where == "encoder.2":
        assert seen == [where, where], "the hook must fire on both routes"
        assert _count(on, "wm_conv64_bf_tail") == 1, "only model.1 -> model.2 may fold"      # encoder.1 -> encoder.2 are two calls
    _all_equal(on, off)


def test_no_grad_in_training_mode(awm, dev, monkeypatch):
    G0, D0 = _models(awm, dev, 16)
    s, msg = _inputs(dev, 16, NET_T, 97)
    on = _step(awm, G0, D0, s, msg, True, monkeypatch, grad=False)
    off = _step(awm, G0, D0, s, msg, False, monkeypatch, grad=False)
    assert on["counts"] == off["counts"] and _count(on, "wm_conv64_bf_tail") == 0 and _count(on, "wm_lstm_fwd_tail") == 0
    _all_equal(on, off)


def test_eval_mode(awm, dev, monkeypatch):
    G0, D0 = _models(awm, dev, 16)
    s, msg = _inputs(dev, 16, NET_T, 99)

    def prepare(G, D):
        G.eval()
        D.eval()
    on = _step(awm, G0, D0, s, msg, True, monkeypatch, prepare=prepare)
    off = _step(awm, G0, D0, s, msg, False, monkeypatch, prepare=prepare)
    assert on["counts"] == off["counts"] and _count(on, "wm_conv64_bf_tail") == 0 and _count(on, "wm_lstm_fwd_tail") == 0
    _all_equal(on, off)
