"""CPU-side checks of the rank-one route's switch (ops._HEAD1_R1, WM_HEAD1_RANK1, ops.set_head1_rank1), of its preconditions and of the
prototypes the header declares for the entry points it calls."""
import torch

import awm_amd
from awm_amd import ops


def test_environment_variable_reading_is_pure():
    assert ops.read_head1_rank1({}) is True
    assert ops.read_head1_rank1({"WM_HEAD1_RANK1": "1"}) is True
    assert ops.read_head1_rank1({"WM_HEAD1_RANK1": "0"}) is False
    assert ops.read_head1_rank1({"WM_HEAD1_RANK1": "yes"}) is False            # only "1" switches a path on, as in read_switches
    assert ops.read_head1_rank1({"WM_TAIL_IN_HEAD": "0"}) is True              # another switch's variable does not move it


def test_setter_and_table():
    before = ops._HEAD1_R1["on"]
    try:
        ops.set_head1_rank1(False)
        assert ops._HEAD1_R1["on"] is False
        ops.set_head1_rank1(1)
        assert ops._HEAD1_R1["on"] is True
    finally:
        ops.set_head1_rank1(before)
    assert not any(env == "WM_HEAD1_RANK1" for _, (_, _, env, *_r) in ops.SWITCHES.items())
    assert ops.read_switches({"WM_HEAD1_RANK1": "0"}) == ops.read_switches({})   # the table does not know the variable


def test_route_needs_a_device_tensor():
    assert not ops.head1_rank1_applies(torch.zeros(2, 64, 128))                # a CPU tensor never takes the route


def test_prototypes():
    protos = awm_amd.lib.protos
    base = protos["wm_dwgrad64_bf"]
    r1 = protos["wm_dwgrad64_bf_r1"]
    assert r1[:len(base) - 1] == base[:-1], "wm_dwgrad64_bf's arguments, in its order"
    assert [n for _, n in r1[len(base) - 1:]] == ["g1", "hw", "stream"]
    assert [n for _, n in protos["wm_relu_bwd_reduce_mask_r1"]] == ["g1", "w", "mask", "y2", "partial", "dzmax", "B", "T", "stream"]
