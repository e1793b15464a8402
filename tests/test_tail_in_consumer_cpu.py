"""CPU-side checks of the tail-in-consumer switch (ops._TAILC, WM_TAIL_IN_CONSUMER, ops.set_tail_in_consumer): its default, its
environment variable, its setter, that it lives outside the SWITCHES table, and that its precondition says no without a GPU tensor.
No GPU call."""
import copy

import pytest
import torch

from awm_amd import ops


@pytest.fixture
def restore():
    before = ops._TAILC["on"]
    yield before
    ops._TAILC["on"] = before


def test_default_and_environment_variable():
    assert ops.read_tail_in_consumer({}) is True
    assert ops.read_tail_in_consumer({"WM_TAIL_IN_CONSUMER": "1"}) is True
    assert ops.read_tail_in_consumer({"WM_TAIL_IN_CONSUMER": "0"}) is False
    assert ops.read_tail_in_consumer({"WM_TAIL_IN_CONSUMER": "yes"}) is False      # only "1" switches a path on, as in read_switches
    assert ops.read_tail_in_consumer({"WM_TAIL_IN_HEAD": "0"}) is True             # another switch's variable does not move it


def test_setter(restore):
    conv, lstm, heads = copy.deepcopy(ops._CONV), copy.deepcopy(ops._LSTM), copy.deepcopy(ops._HEADS)
    ops.set_tail_in_consumer(False)
    assert ops._TAILC["on"] is False
    ops.set_tail_in_consumer(1)
    assert ops._TAILC["on"] is True
    assert ops._CONV == conv and ops._LSTM == lstm and ops._HEADS == heads          # it moves nothing else


def test_switch_table_and_stores_unchanged():
    assert len(ops.SWITCHES) == 16
    assert not any("tail" in name or env == "WM_TAIL_IN_CONSUMER" for name, (_, _, env, *_r) in ops.SWITCHES.items())
    assert set(ops._CONV) == {"bf16x6", "schedule", "one_launch_eval", "fused_bwd", "mask_on_load", "pair_fold", "bwd_f16x3", "fwd_f16x3",
                              "conv7_f16x3", "eval_f16x3"}
    assert set(ops._LSTM) == {"fused", "bwd_fused", "bwd_ws", "fwd_ws"}
    got = ops.read_switches({"WM_TAIL_IN_CONSUMER": "0"})
    assert got == ops.read_switches({})                                             # the table does not know the variable


def test_precondition_needs_a_gpu_frame(restore):
    ops.set_tail_in_consumer(True)
    x = torch.zeros(2, 64, 256, requires_grad=True)
    assert ops.tail_in_consumer_applies(x) is False and ops.tail_in_consumer_applies(x, lstm=True) is False
    assert ops.tail_in_consumer_applies(torch.zeros(64, 256)) is False
