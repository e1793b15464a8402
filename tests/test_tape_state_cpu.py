"""CPU-side checks of the tape's named state in ops.py -- BlockParams, BlockSaved, LstmSaved, the one function that lines a block's
gradients up with its parameters, and the mode check of _resblock_bwd_fused -- and a dry run of four nodes on CPU tensors: a stub
records the C-ABI calls, nothing is computed, and every parameter's .grad must be the tensor the recorded launch was handed as that
parameter's destination.  No GPU call."""
import pytest
import torch

import awm_amd
from awm_amd import ops
from awm_amd.modules import _rb_args

B, T = 2, 128
# the launches that exist only for the routes a CPU tensor must never take (each of them asks x.is_cuda)
FUSED_ROUTES = {"wm_conv64_bf_tail", "wm_conv64_bf_stem", "wm_dwgrad64_bf_stem", "wm_dwgrad64_bf_r1", "wm_relu_bwd_reduce_mask_r1"}
# where a launch takes its gradient destinations (0 = the entry point's first argument, include/wm_hip.h)
DW, DB = 15, 16                      # wm_dwgrad64_bf: dw, dbias
DG, DBE = 9, 10                      # wm_bn_bwd_finalize: dgamma, dbeta


def test_field_orders():
    assert ops.BlockParams._fields == ("w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2", "rm1", "rv1", "nbt1", "rm2", "rv2", "nbt2")
    assert ops.BlockSaved._fields == ("x", "y1", "y2", "mask", "cst", "w1", "w2", "g1", "g2")
    assert ops.LstmSaved._fields == ("x", "h", "gates", "cst", "w_ih", "w_hh")
    for cls in (ops.BlockParams, ops.BlockSaved, ops.LstmSaved):
        assert issubclass(cls, tuple)


def test_block_saved_is_still_a_tuple_and_names_the_bn2_constants():
    cst = torch.arange(8.0).reshape(8, 1).repeat(1, 64)
    saved = ops.BlockSaved("x", "y1", "y2", None, cst, "w1", "w2", "g1", "g2")
    assert len(saved) == 9 and saved[:3] == ("x", "y1", "y2") and tuple(saved)[3] is None
    assert torch.equal(saved.sc2, cst[4]) and torch.equal(saved.sh2, cst[5])
    assert saved.sc2.data_ptr() == cst[4].data_ptr() and saved.sh2.data_ptr() == cst[5].data_ptr()        # views, not copies
    patched = saved._replace(mask="m")
    assert tuple(patched) == ("x", "y1", "y2", "m", cst, "w1", "w2", "g1", "g2") and saved.mask is None
    assert [float(r[0]) for r in ops._bn_consts(cst)] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    with pytest.raises(AttributeError):
        saved.sc2 = cst[0]


def test_rb_args_matches_block_params():
    m = awm_amd.ResBlock(64)
    c1, n1, _, c2, n2 = m.block
    p = _rb_args(m)
    assert type(p) is ops.BlockParams and len(p) == 14
    want = dict(w1=c1.weight, b1=c1.bias, g1=n1.weight, be1=n1.bias, w2=c2.weight, b2=c2.bias, g2=n2.weight, be2=n2.bias,
                rm1=n1.running_mean, rv1=n1.running_var, nbt1=n1.num_batches_tracked,
                rm2=n2.running_mean, rv2=n2.running_var, nbt2=n2.num_batches_tracked)
    assert set(want) == set(p._fields)
    for name, t in want.items():
        assert getattr(p, name) is t, name
    assert all(a is b for a, b in zip(p, (want[n] for n in ops.BlockParams._fields)))


def test_gradients_line_up_with_the_parameters():
    names = ("dw1", "db1", "dg1", "dbe1", "dw2", "db2", "dg2", "dbe2")
    out = ops._block_grads(names)
    assert len(out) == 14 and isinstance(out, tuple)
    for grad, param in zip(names, ("w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2")):
        assert out[ops.BlockParams._fields.index(param)] == grad
    for buf in ("rm1", "rv1", "nbt1", "rm2", "rv2", "nbt2"):
        assert out[ops.BlockParams._fields.index(buf)] is None
    assert tuple(out) == names + (None, None, None, None, None, None)
    assert tuple(ops._block_grads(list(names))) == tuple(out)            # (a backward unpacks them into a list)


def test_cut_names_a_nodes_arguments_and_saved_tensors():
    args = tuple(range(14)) + tuple(range(100, 114)) + ("a", "b")
    p1, p2, rest = ops._cut(args, ops.BlockParams, ops.BlockParams)
    assert type(p1) is type(p2) is ops.BlockParams and tuple(p1) == args[:14] and tuple(p2) == args[14:28] and rest == ("a", "b")
    p, rest = ops._cut(args[:15], ops.BlockParams)
    assert tuple(p) == args[:14] and rest == (100,)
    saved = list(range(9)) + list(range(20, 29)) + list(range(40, 46)) + ["s", "w", "b"]          # EncoderLSTMFn's order, behind a stem
    first, second, lstm, stem = ops._cut(saved, ops.BlockSaved, ops.BlockSaved, ops.LstmSaved)
    assert (type(first), type(second), type(lstm)) == (ops.BlockSaved, ops.BlockSaved, ops.LstmSaved)
    assert first.mask == 3 and second.x == 20 and second.cst == 24 and lstm.gates == 42 and stem == ("s", "w", "b")
    assert ops._cut(saved[:24], ops.BlockSaved, ops.BlockSaved, ops.LstmSaved)[-1] == ()
    with pytest.raises(TypeError):
        ops._cut(args[:13], ops.BlockParams)                                 # a miscounted argument list does not pass
    with pytest.raises(TypeError):
        ops.BlockParams(*args[:8])                                           # the buffers have no defaults


# ------------------------------------------------------------------------------------------------ the dry run
@pytest.fixture
def recorder(monkeypatch):
    calls = []

    class Recorder:
        def __getattr__(self, name):
            if not name.startswith("wm_"):
                raise AttributeError(name)
            return lambda *a: calls.append((name,) + a)
    monkeypatch.setattr(ops, "lib", Recorder())
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_chk", lambda t, name, ndim=None, dtype=torch.float32: t.contiguous())
    monkeypatch.setitem(ops._ASYNC, "on", False)
    monkeypatch.setitem(ops._LSTM_DX, "in_bwd", True)
    monkeypatch.setitem(ops._STEMC, "on", True)
    monkeypatch.setitem(ops._HEAD1_R1, "on", True)
    with ops.switches(bf16x6=True, fused_bwd=True, mask_on_load=True, bwd_f16x3=True, fwd_f16x3=True, pair_fold=True,
                      lstm_fused=True, lstm_bwd_ws=True, lstm_bwd_fused=False):
        yield calls


def _named(calls, name):
    return [c[1:] for c in calls if c[0] == name]


def _check_block(calls, block, pair, finalize):
    """block's eight gradients against the `pair`-th / `finalize`-th launches of its backward: (conv2, conv1) and (BN2, BN1)"""
    c1, n1, _, c2, n2 = block.block
    dw = _named(calls, "wm_dwgrad64_bf")
    bn = _named(calls, "wm_bn_bwd_finalize")
    for conv, norm, i, j in ((c2, n2, pair[0], finalize[0]), (c1, n1, pair[1], finalize[1])):
        assert conv.weight.grad.data_ptr() == dw[i][DW] and conv.bias.grad.data_ptr() == dw[i][DB]
        assert norm.weight.grad.data_ptr() == bn[j][DG] and norm.bias.grad.data_ptr() == bn[j][DBE]
        assert conv.weight.grad.shape == conv.weight.shape and norm.bias.grad.shape == (64,)
    ptrs = [p.grad.data_ptr() for p in block.parameters()]
    assert len(set(ptrs)) == 8                                               # eight destinations, no two the same tensor
    assert all(b.grad is None for b in block.buffers())


def _lstm():
    lstm = torch.nn.LSTM(64, 64, batch_first=True)
    return lstm, (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)


def test_resblock_node(recorder):
    block = awm_amd.ResBlock(64)
    x = torch.rand(B, 64, T, requires_grad=True)
    y = block(x)
    assert type(y.grad_fn).__name__.startswith("ResBlockFn") and len(y.grad_fn.saved_tensors) == 9
    y.backward(torch.rand_like(y))
    names = [c[0] for c in recorder]
    assert not FUSED_ROUTES & set(names)
    assert names.count("wm_dwgrad64_bf") == 2 and names.count("wm_bn_bwd_finalize") == 2
    _check_block(recorder, block, pair=(0, 1), finalize=(0, 1))
    assert x.grad.data_ptr() == _named(recorder, "wm_dwgrad64_bf")[1][12]    # dx leaves the conv1 pair


def test_resblock_head1_node_on_the_unfused_route(recorder):
    block, head = awm_amd.ResBlock(64), torch.nn.Conv1d(64, 1, 1)
    x = torch.rand(B, 64, T, requires_grad=True)
    y = ops.ResBlockHead1Fn.apply(x, *_rb_args(block), head.weight, head.bias)
    assert len(y.grad_fn.saved_tensors) == 11 and y.shape == (B, 1, T)
    del recorder[:]
    y.backward(torch.rand_like(y))
    names = [c[0] for c in recorder]
    assert not FUSED_ROUTES & set(names)
    (hb,) = _named(recorder, "wm_head1_bwd")
    assert hb[3] is not None                                                 # the gradient frame is written: not the rank-one route
    assert names.index("wm_head1_bwd") < names.index("wm_relu_bwd_reduce_mask")
    assert head.weight.grad.data_ptr() == hb[5] and head.bias.grad.data_ptr() == hb[6]
    assert hb[3] == _named(recorder, "wm_relu_bwd_reduce_mask")[0][0]        # ... and the block's backward reads it
    _check_block(recorder, block, pair=(0, 1), finalize=(0, 1))
    assert x.grad.data_ptr() == _named(recorder, "wm_dwgrad64_bf")[1][12]


def test_lstm_node(recorder):
    lstm, params = _lstm()
    x = torch.rand(B, 64, T, requires_grad=True)
    y = ops.LSTMFn.apply(x, *params)
    assert len(y.grad_fn.saved_tensors) == 6
    del recorder[:]
    y.backward(torch.rand_like(y))
    assert [c[0] for c in recorder] == ["wm_lstm_bwd_wgrad", "wm_lstm_dx"]
    assert tuple(p.grad.data_ptr() for p in params) == recorder[0][8:12]
    assert x.grad.data_ptr() == recorder[1][3]


def test_encoder_lstm_node(recorder):
    e1, e2 = awm_amd.ResBlock(64), awm_amd.ResBlock(64)
    lstm, params = _lstm()
    x = torch.rand(B, 64, T, requires_grad=True)
    y = ops.EncoderLSTMFn.apply(x, *_rb_args(e1), *_rb_args(e2), *params)
    assert "wm_lstm_fwd_tail" in [c[0] for c in recorder] and not FUSED_ROUTES & {c[0] for c in recorder}
    assert len(y.grad_fn.saved_tensors) == 24
    del recorder[:]
    y.backward(torch.rand_like(y))
    names = [c[0] for c in recorder]
    assert not FUSED_ROUTES & set(names)
    assert names[0] == "wm_lstm_bwd_wgrad_dx" and names.count("wm_dwgrad64_bf") == 4 and names.count("wm_bn_bwd_finalize") == 4
    assert names.count("wm_relu_bwd_reduce_mask") == 1                       # the second block folds the first block's
    assert tuple(p.grad.data_ptr() for p in params) == recorder[0][9:13]
    _check_block(recorder, e2, pair=(0, 1), finalize=(0, 1))                 # the backward runs the second block first
    _check_block(recorder, e1, pair=(2, 3), finalize=(2, 3))
    pairs = _named(recorder, "wm_dwgrad64_bf")
    assert [p[20] for p in pairs] == [1, 8, 1, 2]                            # epilogues: conv2, conv1 + fold, conv2, conv1
    assert x.grad.data_ptr() == pairs[3][12]


# ------------------------------------------------------------------------------------------------ _resblock_bwd_fused's modes
def _saved_block():
    f = torch.rand(B, 64, T)
    return (f, f.clone(), f.clone(), torch.zeros(B * 64 * (T // 32), dtype=torch.int32), torch.rand(8, 64), torch.rand(64, 64, 3),
            torch.rand(64, 64, 3), torch.rand(64), torch.rand(64)), torch.rand(B, 64, T)


def test_fused_backward_rejects_modes_that_exclude_each_other(recorder):
    saved, g = _saved_block()
    rank1 = (torch.rand(B, 1, T), torch.rand(1, 64, 1))
    stem = (torch.rand(B, 1, T), torch.rand(64, 1, 7), torch.rand(64))
    pre = (torch.rand(ops.NCU, 2, 64), torch.rand(ops.NCU))
    with pytest.raises(ValueError, match="rank1"):
        ops._resblock_bwd_fused(saved, True, None, rank1=rank1, fold=(saved[3], saved[2]))
    with pytest.raises(ValueError, match="rank1"):
        ops._resblock_bwd_fused(saved, True, None, rank1=rank1, pre=pre)
    with pytest.raises(ValueError, match="stem"):
        ops._resblock_bwd_fused(saved, True, g, stem=stem)
    assert recorder == []                                                    # refused before anything was launched
    dx, grads, fout = ops._resblock_bwd_fused(saved, True, g, pre=pre, stem=stem)          # a plain 9-tuple, a legal combination
    assert len(grads) == 8 and fout is None and dx.shape == g.shape
    assert [c[0] for c in recorder if c[0].startswith("wm_dwgrad")] == ["wm_dwgrad64_bf", "wm_dwgrad64_bf_stem"]
