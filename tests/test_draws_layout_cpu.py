"""Where the attack layer lives (no GPU): draws.py (the host-side draws and the table of output words) <- attacks_host.py (what a CPU
tensor runs) <- attacks.py (the modules and the evaluation loops), with every moved name still reachable as attacks.<name>; and the
table draws.WORDS itself: what it holds, that no two counters meet, and that every affine-mapped parameter is drawn from the word the
table names -- computed with tests/draw_yardstick.py, which has nothing of the package in it.

A new attack adds its cell to WORDS_EXPECTED below and, if it maps a pair onto its word, its row to DRAWN."""
import types

import numpy as np
import pytest
import torch

import draw_yardstick as Y
from awm_amd import attacks, attacks_host, draws, dsp

# every name that left attacks.py, by the module that defines it now
DRAWS_NAMES = [
    "_M0", "_M1", "_W0", "_W1", "FAMILIES", "philox4x32_10", "_unit", "_key", "_words", "_affine",
    "normal_noise", "_normals",
    "row_parameters", "row_snr_db", "row_lpc_snr_db", "row_reduce_db",
    "row_reverb_params", "row_bank_index", "rir_taps",
    "row_warp_params", "row_stretch_rates", "row_pitch_params",
    "_check_cut", "row_splice_spans", "SPLICE_KINDS",
]
HOST_NAMES = [
    "_lpc_rows_host", "_conv_rows_host", "_sinpi", "_warp_rows_host", "_wsola_rows_host", "_gather_ext",
    "splice_rows_host", "pack_labels", "unpack_labels",
]
STAYED = [
    "NOISE_GRAD_MODES", "_pair", "_RowDraws", "Distortion", "Lowpass", "Resampled", "TransformCodec", "LpcCodec", "NoiseSuppress",
    "Convolved", "Reverb", "TimeWarp", "TimeStretch", "PitchShift", "Splice", "echo_ir", "code_entropy_kbps", "localization_metrics",
    "evaluate_localization", "evaluate_robustness", "evaluate_robustness_by_class",
]

SPANS = 8
WORDS_EXPECTED = {
    ("param", 0): "Distortion.gain_db", ("param", 1): "Distortion.snr_db", ("param", 2): "Distortion.noisy",
    ("param", 3): "TransformCodec.snr_db",
    ("param2", 0): "Reverb.rt60", ("param2", 1): "Reverb.drr_db", ("param2", 2): "Convolved.bank", ("param2", 3): "LpcCodec.snr_db",
    ("warp", 0): "TimeWarp.speed", ("warp", 1): "TimeWarp.shift_s", ("warp", 2): "TimeWarp.flutter_hz",
    ("warp", 3): "TimeWarp.flutter_depth",
    ("warp_phase", 0): "TimeWarp.phase", ("warp_phase", 1): "TimeStretch.rate", ("warp_phase", 2): "PitchShift.semitones",
    ("warp_phase", 3): "NoiseSuppress.reduce_db",
}
for _j in range(SPANS):
    WORDS_EXPECTED.update({(f"splice_span{_j}", 0): f"Splice.coin[{_j}]", (f"splice_span{_j}", 1): f"Splice.length[{_j}]",
                           (f"splice_span{_j}", 2): f"Splice.start[{_j}]", (f"splice_span{_j}", 3): f"Splice.kind[{_j}]",
                           (f"splice_shift{_j}", 0): f"Splice.shift[{_j}]"})          # words 1..3 of splice_shift{j} are free


def test_attacks_hands_on_the_same_objects():
    for n in DRAWS_NAMES:
        assert getattr(attacks, n) is getattr(draws, n), n
    for n in HOST_NAMES:
        assert getattr(attacks, n) is getattr(attacks_host, n), n
    assert attacks.WORDS is draws.WORDS
    assert len(set(DRAWS_NAMES + HOST_NAMES + STAYED)) == len(DRAWS_NAMES) + len(HOST_NAMES) + len(STAYED)


def test_where_the_definitions_live():
    for n in DRAWS_NAMES:
        f = getattr(draws, n)
        if callable(f):
            assert f.__module__.endswith(".draws"), n
    for n in HOST_NAMES:
        assert getattr(attacks_host, n).__module__.endswith(".attacks_host"), n
    for n in STAYED:
        f = getattr(attacks, n)
        if callable(f):
            assert f.__module__.endswith(".attacks"), n
    assert attacks.row_snr_db.__module__.endswith(".draws") and attacks._lpc_rows_host.__module__.endswith(".attacks_host")
    assert attacks.Distortion.__module__.endswith(".attacks")
    # the two methods the CPU path and tests/test_mdct_codec_cpu.py call are still there, and hand on to the free functions
    assert attacks_host.distort_rows_host.__module__.endswith(".attacks_host")
    assert attacks_host.mdct_codec_rows_host.__module__.endswith(".attacks_host")
    assert callable(attacks.Distortion._host) and callable(attacks.TransformCodec._host)


def test_imports_go_one_way():
    import awm_amd
    assert awm_amd.attacks is attacks and awm_amd.draws is draws
    allowed = {draws: (dsp,), attacks_host: (dsp, draws)}
    for low, may in allowed.items():
        for name, v in vars(low).items():
            assert v is not attacks, f"{low.__name__}.{name} is the module attacks"
            if isinstance(v, types.ModuleType) and v.__name__.startswith("awm_amd"):
                assert any(v is m for m in may), f"{low.__name__} imports {v.__name__}"
    assert draws.dsp is dsp


def test_rows_come_with_their_numbers():
    m = attacks._RowDraws(0)
    x, rows, numbers = m._rows(torch.zeros(3, 1, 8), 2 ** 32 - 3)
    assert rows == 3 and numbers.tolist() == [2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1] and tuple(x.shape) == (3, 1, 8)
    with pytest.raises(ValueError):
        m._rows(torch.zeros(3, 1, 8), 2 ** 32 - 2)


def test_the_table_is_todays_allocation():
    assert draws.WORDS == WORDS_EXPECTED and len(WORDS_EXPECTED) == 16 + 5 * SPANS
    assert dsp.SPLICE_MAX_SPANS == SPANS
    owners = list(draws.WORDS.values())
    assert len(set(owners)) == len(owners), "one owner per word, one word per owner"
    for family, index in draws.WORDS:
        assert family in draws.FAMILIES and draws.FAMILIES[family][0] is not None, family
        assert isinstance(index, int) and 0 <= index <= 3, (family, index)


def test_the_counters_do_not_collide():
    counters = list(draws.FAMILIES.values())
    assert len(set(counters)) == len(counters)
    counting = {f: c for f, c in draws.FAMILIES.items() if c[0] is None}
    assert counting == {"sample": (None, 0), "rir_tap": (None, 0xFFFFFFFE)}
    for family, (w0, w1) in draws.FAMILIES.items():
        if family not in counting:
            assert w1 == 0xFFFFFFFF and 0 <= w0 <= 0xFFFFFFFF, family       # word 1 apart from both counting families': no meeting
    # the yardstick's list is the parameter families', word for word
    assert {f: c for f, c in draws.FAMILIES.items() if f not in counting} == Y.FAMILIES
    assert {f for f, _ in draws.WORDS} == set(Y.FAMILIES)


SEEDS = ((7 << 32) + 11, (1 << 63) + (3 << 32) + 5)       # the second has bit 63 set
DRAWS = (0, 2 ** 32 - 1)
ROWS = (5 + np.arange(8), np.array([2 ** 32 - 1]))
PAIR = {"gain_db": (-6.0, 6.0), "snr_db": (10.0, 30.0), "rt60": (0.1, 0.4), "drr_db": (0.0, 12.0), "speed": (0.8, 1.25),
        "shift_s": (-0.01, 0.02), "flutter_hz": (0.5, 8.0), "flutter_depth": (0.0, 0.25), "rate": (0.9, 1.1), "semitones": (-1.0, 1.0),
        "reduce_db": (6.0, 24.0)}


def _warp(s, d, r):
    # sample_rate 1: off = shift and w = flutter rate, each the float32 draw itself
    return draws.row_warp_params(s, d, r, PAIR["speed"], PAIR["shift_s"], PAIR["flutter_hz"], PAIR["flutter_depth"], 1)


# owner -> the value the package draws for it, as the float32 array the affine map gives
DRAWN = {
    "Distortion.gain_db": lambda s, d, r: draws.row_parameters(s, d, r, (*PAIR["gain_db"], *PAIR["snr_db"], 0.5))[0],
    "Distortion.snr_db": lambda s, d, r: draws.row_parameters(s, d, r, (*PAIR["gain_db"], *PAIR["snr_db"], 0.5))[1],
    "TransformCodec.snr_db": lambda s, d, r: draws.row_snr_db(s, d, r, PAIR["snr_db"]),
    "LpcCodec.snr_db": lambda s, d, r: draws.row_lpc_snr_db(s, d, r, PAIR["snr_db"]),
    "Reverb.rt60": lambda s, d, r: draws.row_reverb_params(s, d, r, PAIR["rt60"], PAIR["drr_db"])[0],
    "Reverb.drr_db": lambda s, d, r: draws.row_reverb_params(s, d, r, PAIR["rt60"], PAIR["drr_db"])[1],
    "TimeWarp.speed": lambda s, d, r: _warp(s, d, r)[:, 0],
    "TimeWarp.shift_s": lambda s, d, r: _warp(s, d, r)[:, 1],
    "TimeWarp.flutter_hz": lambda s, d, r: _warp(s, d, r)[:, 3],
    "TimeStretch.rate": lambda s, d, r: draws.row_stretch_rates(s, d, r, PAIR["rate"]),
    "PitchShift.semitones": lambda s, d, r: draws.row_pitch_params(s, d, r, PAIR["semitones"])[0],
    "NoiseSuppress.reduce_db": lambda s, d, r: draws.row_reduce_db(s, d, r, PAIR["reduce_db"]),
}
CELL = {owner: cell for cell, owner in WORDS_EXPECTED.items()}


def _from_the_table(owner, seed, draw, rows):
    """affine32 of the word the TABLE names for `owner`, from the yardstick's generator and the yardstick's counters"""
    family, index = CELL[owner]
    w = Y.philox4x32_10((*Y.FAMILIES[family], rows.astype(np.uint64), draw), Y.key_of(seed))[index]
    return Y.affine32(PAIR[owner.split(".")[1]], Y.unit(w))


def _same_bits(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), what


@pytest.mark.parametrize("owner", sorted(DRAWN))
def test_the_table_is_what_the_functions_do(owner):
    for seed in SEEDS:
        for draw in DRAWS:
            for rows in ROWS:
                _same_bits(np.ascontiguousarray(DRAWN[owner](seed, draw, rows)), _from_the_table(owner, seed, draw, rows),
                           (owner, seed, draw, rows))


def test_flutter_depth_is_drawn_from_its_word():
    """TimeWarp hands the depth on only inside d and c: c = min(1, 1 / (a (1 + depth))) in float64 from the float32 draws, rounded once
    (row_warp_params's definition), so the depth the table names must give the package's c, and another word's would not"""
    for seed in SEEDS:
        for draw in DRAWS:
            for rows in ROWS:
                a = _from_the_table("TimeWarp.speed", seed, draw, rows).astype(np.float64)
                depth = _from_the_table("TimeWarp.flutter_depth", seed, draw, rows).astype(np.float64)
                want = np.minimum(1.0, 1.0 / (a * (1.0 + depth))).astype(np.float32)
                _same_bits(np.ascontiguousarray(_warp(seed, draw, rows)[:, 5]), want, (seed, draw, rows))
    assert set(DRAWN) | {"TimeWarp.flutter_depth"} == {o for o in CELL if o.split(".")[1] in PAIR}, "every affine-mapped owner is checked"
