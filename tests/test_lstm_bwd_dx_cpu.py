"""CPU-side checks of the dx-inside-the-BPTT switch (ops._LSTM_DX, WM_LSTM_DX_IN_BWD, ops.set_lstm_dx_in_bwd), of the prototype the
binding reads from the header, and of the call ops._lstm_bwd makes under it: a stub records the C-ABI calls, nothing is computed."""
import copy

import pytest
import torch

from awm_amd import _lib, ops


@pytest.fixture
def restore():
    before = ops._LSTM_DX["in_bwd"]
    yield before
    ops._LSTM_DX["in_bwd"] = before


def test_default_and_environment_variable():
    assert ops.read_lstm_dx_in_bwd({}) is True
    assert ops.read_lstm_dx_in_bwd({"WM_LSTM_DX_IN_BWD": "1"}) is True
    assert ops.read_lstm_dx_in_bwd({"WM_LSTM_DX_IN_BWD": "0"}) is False
    assert ops.read_lstm_dx_in_bwd({"WM_LSTM_DX_IN_BWD": "yes"}) is False          # only "1" switches a path on, as in read_switches
    assert ops.read_lstm_dx_in_bwd({"WM_LSTM_BWD_WS": "0"}) is True                # another switch's variable does not move it


def test_setter_and_switch_table(restore):
    lstm = copy.deepcopy(ops._LSTM)
    ops.set_lstm_dx_in_bwd(False)
    assert ops._LSTM_DX["in_bwd"] is False
    ops.set_lstm_dx_in_bwd(1)
    assert ops._LSTM_DX["in_bwd"] is True
    assert ops._LSTM == lstm                                                        # it moves nothing else
    assert not any(env == "WM_LSTM_DX_IN_BWD" for _, (_, _, env, *_r) in ops.SWITCHES.items())
    assert ops.read_switches({"WM_LSTM_DX_IN_BWD": "0"}) == ops.read_switches({})   # the table does not know the variable


def test_prototype_in_the_header():
    proto = _lib.parse_header()["wm_lstm_bwd_wgrad_dx"]
    assert [n for _, n in proto] == ["gates", "cst", "dh_out", "w_hh", "w_ih", "x", "h", "partial", "dw_ih", "dw_hh", "db_ih", "db_hh",
                                     "dx", "B", "T", "accumulate", "stream"]
    assert [t for t, _ in proto[:7]] == ["const float*"] * 7 and [t for t, _ in proto[7:13]] == ["float*"] * 6
    assert [t for t, _ in proto[13:]] == ["int", "int", "int", "wm_stream_t"]
    old = _lib.parse_header()["wm_lstm_bwd_wgrad"]
    assert len(old) == 15 and [n for _, n in old[7:11]] == ["dw_ih", "dw_hh", "db_ih", "db_hh"]       # the older entry point stays


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
    return calls


def _saved(T):
    B = 2
    x, h = torch.rand(B, 64, T), torch.rand(B, 64, T)
    return (x, h, torch.rand(B, T, 256), torch.rand(B, T, 64), torch.rand(256, 64), torch.rand(256, 64)), torch.rand(B, 64, T)


def test_the_call_carries_destinations_and_dx(recorder):
    saved, dh = _saved(128)
    x, h, gates, cst, w_ih, w_hh = saved
    with ops.switches(lstm_bwd_ws=True, lstm_bwd_fused=False):
        dx, *dst = ops._lstm_bwd(saved, (None,) * 4, dh, dx_inside=True)
    assert [c[0] for c in recorder] == ["wm_lstm_bwd_wgrad_dx"]
    a = recorder[0][1:]
    assert len(a) == 17
    assert a[:7] == (gates.data_ptr(), cst.data_ptr(), dh.data_ptr(), w_hh.data_ptr(), w_ih.data_ptr(), x.data_ptr(), h.data_ptr())
    assert a[8:12] == tuple(t.data_ptr() for t in dst) and a[12] == dx.data_ptr()
    assert [tuple(t.shape) for t in dst] == [(256, 64), (256, 64), (256,), (256,)] and dx.shape == x.shape
    assert a[13:16] == (2, 128, 0)


def test_flat_store_destinations_keep_the_two_launches(recorder, monkeypatch):
    """side-stream weight gradients on: the destinations are the flat store's views, at positions 8..11 of wm_lstm_bwd_wgrad as ever"""
    monkeypatch.setitem(ops._ASYNC, "on", True)
    saved, dh = _saved(128)
    flat = tuple(torch.zeros(s) for s in ((256, 64), (256, 64), (256,), (256,)))
    with ops.switches(lstm_bwd_ws=True, lstm_bwd_fused=False):
        out = ops._lstm_bwd(saved, flat, dh, dx_inside=True)
    assert [c[0] for c in recorder] == ["wm_lstm_bwd_wgrad", "wm_lstm_dx"]
    assert recorder[0][8:12] == tuple(t.data_ptr() for t in flat) and recorder[0][-2] == 1 and out[1:] == (None,) * 4


@pytest.mark.parametrize("T,switches,inside,want", [
    (128, dict(lstm_bwd_ws=True, lstm_bwd_fused=False), False, ["wm_lstm_bwd_wgrad", "wm_lstm_dx"]),
    (128, dict(lstm_bwd_ws=False, lstm_bwd_fused=False), True, ["wm_lstm_bwd", "wm_lstm_dx", "wm_lstm_wgrad"]),
    (128, dict(lstm_bwd_ws=True, lstm_bwd_fused=True), True, ["wm_lstm_bwd_fused", "wm_lstm_wgrad"]),
    (48, dict(lstm_bwd_ws=True, lstm_bwd_fused=False), True, ["wm_lstm_bwd", "wm_lstm_dx", "wm_lstm_wgrad"]),
    (32, dict(lstm_bwd_ws=True, lstm_bwd_fused=False), True, ["wm_lstm_bwd", "wm_lstm_dx", "wm_lstm_wgrad"]),
])
def test_every_other_condition_keeps_its_launches(recorder, T, switches, inside, want):
    saved, dh = _saved(T)
    with ops.switches(**switches):
        ops._lstm_bwd(saved, (None,) * 4, dh, dx_inside=inside)
    assert [c[0] for c in recorder] == want
