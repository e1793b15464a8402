"""CPU-side checks of the stem-in-conv1 route's switch (ops._STEMC, WM_STEM_IN_CONV1, ops.set_stem_in_conv1), of its preconditions and
of the prototypes the header declares for the two entry points it calls."""
import torch

import awm_amd
from awm_amd import ops


def test_environment_variable_reading_is_pure():
    assert ops.read_stem_in_conv1({}) is True
    assert ops.read_stem_in_conv1({"WM_STEM_IN_CONV1": "1"}) is True
    assert ops.read_stem_in_conv1({"WM_STEM_IN_CONV1": "0"}) is False
    assert ops.read_stem_in_conv1({"WM_STEM_IN_CONV1": "yes"}) is False          # only "1" switches a path on, as in read_switches
    assert ops.read_stem_in_conv1({"WM_TAIL_IN_CONSUMER": "0"}) is True          # another switch's variable does not move it


def test_setter_and_table():
    before = ops._STEMC["on"]
    try:
        ops.set_stem_in_conv1(False)
        assert ops._STEMC["on"] is False
        ops.set_stem_in_conv1(1)
        assert ops._STEMC["on"] is True
    finally:
        ops.set_stem_in_conv1(before)
    assert not any(env == "WM_STEM_IN_CONV1" for _, (_, _, env, *_r) in ops.SWITCHES.items())
    assert ops.read_switches({"WM_STEM_IN_CONV1": "0"}) == ops.read_switches({})   # the table does not know the variable


def test_route_needs_a_device_tensor():
    assert not ops.stem_in_conv1_applies(torch.zeros(2, 1, 128))                 # a CPU tensor never takes the route
    assert not ops.stem_in_conv1_applies(torch.zeros(2, 1, 128), lstm=True)


def test_prototypes():
    protos = awm_amd.lib.protos
    tail = protos["wm_conv64_bf_tail"]
    stem = protos["wm_conv64_bf_stem"]
    assert [n for _, n in stem] == ["s", "stem_w", "stem_b", "wpb_h", "bias", "y0", "y", "stats", "B", "T", "stream"]
    assert stem[-5:] == tail[-5:], "y, stats, B, T, stream as wm_conv64_bf_tail declares them"
    assert [c for c, n in stem if n in ("s", "stem_w", "stem_b", "bias")] == ["const float*"] * 4
    base = dict((n, c) for c, n in protos["wm_dwgrad64_bf"])
    dws = protos["wm_dwgrad64_bf_stem"]
    assert [n for _, n in dws] == ["g", "g2", "ga", "gb", "gc", "wpb", "e1", "y", "partial", "dw", "dbias", "B", "T", "accumulate", "gscale",
                                   "dzmax", "s", "stem_w", "stem_b", "stream"]
    for c, n in dws[:16] + dws[-1:]:
        assert base[n] == c, f"{n}: the type wm_dwgrad64_bf declares"
    assert [c for c, _ in dws[16:19]] == ["const float*"] * 3
