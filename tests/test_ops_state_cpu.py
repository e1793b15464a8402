"""CPU-side checks of the host state in ops.py: the one table of path switches (defaults, environment variables, setters,
the switches() context manager) and the train-step body shared by step.train_step and main14b_2.train_step.  No GPU call."""
import copy

import pytest

import awm_amd
from awm_amd import main14b_2, ops, step

# what the package starts with when no WM_* variable is set -- written out here, not read from ops.SWITCHES
DEFAULTS = {
    "conv": {"bf16x6": True, "schedule": 2, "one_launch_eval": True, "fused_bwd": True, "mask_on_load": True, "pair_fold": True,
             "bwd_f16x3": True, "fwd_f16x3": True, "conv7_f16x3": True, "eval_f16x3": True},
    "lstm": {"fused": True, "bwd_fused": False, "bwd_ws": True, "fwd_ws": True},
    "gconv": {"f16x3": True},
    "main14b_2": {"_FUSED_STRIDED_DGRAD": True},               # a global of that module
    "library": [],
}
# environment variable -> the one (store, key) it sets
VARIABLES = {
    "WM_CONV_BF16X6": ("conv", "bf16x6"), "WM_RESBLOCK_ONE_LAUNCH": ("conv", "one_launch_eval"), "WM_FUSED_BWD": ("conv", "fused_bwd"),
    "WM_MASK_ON_LOAD": ("conv", "mask_on_load"), "WM_PAIR_FOLD": ("conv", "pair_fold"), "WM_BWD_F16X3": ("conv", "bwd_f16x3"),
    "WM_FWD_F16X3": ("conv", "fwd_f16x3"), "WM_CONV7_F16X3": ("conv", "conv7_f16x3"), "WM_EVAL_F16X3": ("conv", "eval_f16x3"),
    "WM_LSTM_FUSED": ("lstm", "fused"), "WM_LSTM_BWD_FUSED": ("lstm", "bwd_fused"), "WM_LSTM_BWD_WS": ("lstm", "bwd_ws"),
    "WM_GCONV_F16X3": ("gconv", "f16x3"), "WM_FUSED_STRIDED_DGRAD": ("main14b_2", "_FUSED_STRIDED_DGRAD"),
}
# public setter -> the (store, key) it sets
SETTERS = {
    "set_conv_bf16x6": ("conv", "bf16x6"), "set_resblock_one_launch": ("conv", "one_launch_eval"), "set_fused_backward": ("conv", "fused_bwd"),
    "set_mask_on_load": ("conv", "mask_on_load"), "set_pair_fold": ("conv", "pair_fold"), "set_bwd_f16x3": ("conv", "bwd_f16x3"),
    "set_fwd_f16x3": ("conv", "fwd_f16x3"), "set_conv7_f16x3": ("conv", "conv7_f16x3"), "set_eval_f16x3": ("conv", "eval_f16x3"),
    "set_lstm_bwd_wave_specialised": ("lstm", "bwd_ws"), "set_gconv_f16x3": ("gconv", "f16x3"),
}


STORES = ("conv", "lstm", "gconv", "main14b_2")


def _stores():
    """the live values, from the objects bench.py and the hot path read: three dicts and main14b_2's module global"""
    return {"conv": ops._CONV, "lstm": ops._LSTM, "gconv": main14b_2._GCONV,
            "main14b_2": {"_FUSED_STRIDED_DGRAD": main14b_2._FUSED_STRIDED_DGRAD}}


def _diff(a, b):
    return {(s, k) for s in STORES for k in a[s] if a[s][k] != b[s][k]}


@pytest.fixture
def restore():
    before = copy.deepcopy(_stores())
    yield before
    for s, d in (("conv", ops._CONV), ("lstm", ops._LSTM), ("gconv", main14b_2._GCONV)):
        d.clear()
        d.update(before[s])
    main14b_2._FUSED_STRIDED_DGRAD = before["main14b_2"]["_FUSED_STRIDED_DGRAD"]


class _FakeLib:
    """stands in for libwm_hip.so: records the two library-backed setters' calls"""

    def __init__(self):
        self.calls = []

    def wm_set_conv_bf_schedule(self, *a):
        self.calls.append(("wm_set_conv_bf_schedule",) + a)

    def wm_set_lstm_fwd_wave_specialised(self, *a):
        self.calls.append(("wm_set_lstm_fwd_wave_specialised",) + a)


def test_defaults():
    assert ops.read_switches({}) == DEFAULTS
    assert set(_stores()["conv"]) == set(DEFAULTS["conv"]) and set(_stores()["lstm"]) == set(DEFAULTS["lstm"])
    assert set(_stores()["gconv"]) == set(DEFAULTS["gconv"]) and isinstance(main14b_2._FUSED_STRIDED_DGRAD, bool)
    assert len(ops.SWITCHES) == sum(len(DEFAULTS[s]) for s in STORES)


@pytest.mark.parametrize("var", sorted(VARIABLES))
def test_each_variable_sets_its_one_switch(var, restore):
    store, key = VARIABLES[var]
    flipped = "0" if DEFAULTS[store][key] else "1"
    got = ops.read_switches({var: flipped})
    assert _diff(got, DEFAULTS) == {(store, key)} and got["library"] == []
    assert got[store][key] is (not DEFAULTS[store][key])
    assert ops.read_switches({var: "1" if DEFAULTS[store][key] else "0"}) == DEFAULTS
    assert ops.read_switches({var: "yes"})[store][key] is False          # only "1" switches a path on
    assert _stores() == restore                                          # pure: the live stores did not move


def test_library_backed_variables(restore):
    got = ops.read_switches({"WM_CONV_BF_SCHEDULE": "0"})
    assert _diff(got, DEFAULTS) == {("conv", "schedule")} and got["conv"]["schedule"] == 0 and got["library"] == ["schedule"]
    got = ops.read_switches({"WM_CONV_BF_SCHEDULE": "2"})
    assert _diff(got, DEFAULTS) == set() and got["library"] == ["schedule"]            # present: still pushed into the library
    got = ops.read_switches({"WM_LSTM_FWD_WS": "0"})
    assert _diff(got, DEFAULTS) == {("lstm", "fwd_ws")} and got["lstm"]["fwd_ws"] is False and got["library"] == ["lstm_fwd_ws"]
    assert _stores() == restore


@pytest.mark.parametrize("name", sorted(SETTERS))
def test_each_setter_sets_its_one_switch(name, restore):
    store, key = SETTERS[name]
    setter = getattr(main14b_2 if store == "gconv" else ops, name)
    for value in (not restore[store][key], restore[store][key]):
        setter(value)
        assert _stores()[store][key] is value
        assert _diff(_stores(), restore) == ({(store, key)} if value != restore[store][key] else set())


def test_library_backed_setters_call_the_library(restore, monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(ops, "lib", fake)
    ops.set_conv_bf_schedule(0)
    assert ops._CONV["schedule"] == 0 and _diff(_stores(), restore) == {("conv", "schedule")}
    ops.set_conv_bf_schedule(2)
    ops.set_lstm_fwd_wave_specialised(False)
    assert ops._LSTM["fwd_ws"] is False and _diff(_stores(), restore) == {("lstm", "fwd_ws")}
    ops.set_lstm_fwd_wave_specialised(True)
    assert fake.calls == [("wm_set_conv_bf_schedule", 0, None), ("wm_set_conv_bf_schedule", 2, None),
                          ("wm_set_lstm_fwd_wave_specialised", 0, None), ("wm_set_lstm_fwd_wave_specialised", 1, None)]


def test_switches_puts_previous_values_back(restore, monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(ops, "lib", fake)
    ops.set_pair_fold(False)                                             # a non-default previous value
    before = copy.deepcopy(_stores())
    with ops.switches(pair_fold=True, lstm_bwd_fused=True, fused_strided_dgrad=False, schedule=0):
        assert ops._CONV["pair_fold"] is True and ops._LSTM["bwd_fused"] is True and ops._CONV["schedule"] == 0
        assert main14b_2._FUSED_STRIDED_DGRAD is False
        with ops.switches(pair_fold=False, lstm_fused=False):            # nesting
            assert ops._CONV["pair_fold"] is False and ops._LSTM["fused"] is False and ops._LSTM["bwd_fused"] is True
        assert ops._CONV["pair_fold"] is True and ops._LSTM["fused"] is True
    assert _stores() == before and ops._CONV["pair_fold"] is False
    assert fake.calls == [("wm_set_conv_bf_schedule", 0, None), ("wm_set_conv_bf_schedule", 2, None)]   # the library followed both ways
    with pytest.raises(ZeroDivisionError):
        with ops.switches(bwd_f16x3=False, gconv_f16x3=False):
            assert ops._CONV["bwd_f16x3"] is False and main14b_2._GCONV["f16x3"] is False
            1 / 0
    assert _stores() == before


def test_switches_rejects_an_unknown_name_before_changing_anything(restore):
    with pytest.raises((KeyError, TypeError)):
        with ops.switches(bwd_f16x3=False, no_such_switch=True):
            pytest.fail("entered the block")
    assert _stores() == restore


# ------------------------------------------------------------------------------------------------ the shared train step
class _Total:
    def __init__(self, log):
        self.log = log

    def backward(self):
        self.log.append("backward")


class _Optimizer:
    def __init__(self, log):
        self.log = log

    def zero_grad(self, set_to_none=True):
        self.log.append("zero_grad")

    def finish_backward(self):
        self.log.append("finish_backward")

    def step(self):
        self.log.append("step")


TRAIN_STEPS = [(step, awm_amd.train_step), (main14b_2, main14b_2.train_step)]


def _run(monkeypatch, module, train_step, log, forward_fails=False, check_fails=False):
    out = {"total": _Total(log)}

    def forward_losses(generator, detector, s, message):
        log.append("forward")
        assert ops.index_check() == "deferred"                           # no mid-step sync inside the forward
        if forward_fails:
            raise RuntimeError("forward failed")
        return out["total"], out

    def check(wait=True, what=""):
        log.append("check")
        assert wait is True
        if check_fails:
            raise IndexError("message id out of range")
    monkeypatch.setattr(module, "forward_losses", forward_losses)
    monkeypatch.setattr(ops, "check_message_ids", check)
    monkeypatch.setitem(ops._CHECK_INDEX, "mode", "sync")
    monkeypatch.setitem(ops._CHECK_INDEX, "pending", ["the flag of this step"])
    try:
        got = train_step("G", "D", _Optimizer(log), "s", "message", grad_sync=lambda: log.append("grad_sync"))
        assert got is out
    finally:
        assert ops.index_check() == "sync"
        log.append("pending dropped" if ops._CHECK_INDEX["pending"] == [] else "pending kept")


@pytest.mark.parametrize("module,train_step", TRAIN_STEPS, ids=["main16", "main14b_2"])
def test_train_step_order(monkeypatch, module, train_step):
    log = []
    _run(monkeypatch, module, train_step, log)
    assert log == ["zero_grad", "forward", "backward", "finish_backward", "grad_sync", "check", "step", "pending kept"]


@pytest.mark.parametrize("module,train_step", TRAIN_STEPS, ids=["main16", "main14b_2"])
def test_train_step_does_not_update_after_a_failed_forward(monkeypatch, module, train_step):
    log = []
    with pytest.raises(RuntimeError, match="forward failed"):
        _run(monkeypatch, module, train_step, log, forward_fails=True)
    assert log == ["zero_grad", "forward", "pending dropped"]


@pytest.mark.parametrize("module,train_step", TRAIN_STEPS, ids=["main16", "main14b_2"])
def test_train_step_does_not_update_after_a_bad_message_id(monkeypatch, module, train_step):
    log = []
    with pytest.raises(IndexError):
        _run(monkeypatch, module, train_step, log, check_fails=True)
    assert log == ["zero_grad", "forward", "backward", "finish_backward", "grad_sync", "check", "pending dropped"]


# ------------------------------------------------------------------------------------------------ queued weight gradients
def test_queued_weight_gradients_keep_their_destinations(monkeypatch, restore):
    """With gradient destinations registered (FlatAdam's side-stream path) the weight-gradient launches of ResBlockFn, ConvT7Fn and
    LSTMFn run later, when the queue is released: each must then still hand the kernel its destinations (accumulate flag set), and
    the nodes must return None for those parameters.  Dry run on the CPU: a stub records the C-ABI calls, nothing is computed."""
    import torch
    calls = []

    class Recorder:
        def __getattr__(self, name):
            if not name.startswith("wm_"):
                raise AttributeError(name)
            return lambda *a: calls.append((name,) + a)

    def release():
        pending, ops._ASYNC["deferred"] = ops._ASYNC["deferred"], []
        for _, fn in pending:
            fn()
    monkeypatch.setattr(ops, "lib", Recorder())
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_chk", lambda t, name, ndim=None, dtype=torch.float32: t.contiguous())
    monkeypatch.setattr(ops, "release_deferred_wgrads", release)
    monkeypatch.setitem(ops._ASYNC, "on", True)
    block, lstm = awm_amd.ResBlock(64), torch.nn.LSTM(64, 64, batch_first=True)
    convt = torch.nn.ConvTranspose1d(64, 64, 7, padding=3)
    params = [p for m in (block, lstm, convt) for p in m.parameters()]
    for p in params:
        p._wm_grad = torch.zeros_like(p)
    for lstm_bwd_ws in (True, False):
        with ops.switches(lstm_bwd_ws=lstm_bwd_ws, lstm_bwd_fused=False, bf16x6=True):
            y = block(torch.rand(2, 64, 128, requires_grad=True))
            y = ops.LSTMFn.apply(y, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)
            y = ops.ConvT7Fn.apply(y, None, convt.weight, convt.bias)
            del calls[:]
            y.backward(torch.rand_like(y))
            assert ops._ASYNC["deferred"] or not lstm_bwd_ws              # something is queued until the release
            release()
        got = {c[0]: c for c in calls}
        c1, bn1, _, c2, bn2 = block.block
        for name, at, dst in (("wm_wgrad64_bf7", 5, (convt.weight, convt.bias)), ("wm_wgrad64_bf", 10, (c1.weight, c1.bias)),
                              ("wm_lstm_bwd_wgrad" if lstm_bwd_ws else "wm_lstm_wgrad", 8 if lstm_bwd_ws else 5,
                               (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0))):
            assert got[name][at:at + len(dst)] == tuple(p._wm_grad.data_ptr() for p in dst), name
        assert [c[-2] for c in calls if c[0] == "wm_wgrad64_bf"] == [3, 3] and got["wm_wgrad64_bf7"][10] == 1      # accumulate
        assert {c[10] for c in calls if c[0] == "wm_wgrad64_bf"} == {c1.weight._wm_grad.data_ptr(), c2.weight._wm_grad.data_ptr()}
        assert all(p.grad is None for m in (c1, c2, lstm, convt) for p in m.parameters())
