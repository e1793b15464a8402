"""The attacks' draws, frozen: every public draw function of the attack layer (draws.py, reached as attacks.<name>) at fixed arguments
against tests/golden/attack_draws.npz, bit for bit.  The file is the package's own output, written at the last commit before the
generator, the unit map and the counter families were gathered into one place each -- so neither the package's restatement nor
tests/draw_yardstick.py can move a draw without this test saying so.  It is never rewritten.
tests/golden/attack_draws_2.npz holds the four draw functions that came after it (LpcCodec's, NoiseSuppress's, TimeStretch's and
PitchShift's), written by `python tests/test_attack_draws_cpu.py --write` at the last commit before they moved into draws.py.  Rewrite
it only for a change that is MEANT to move draws."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "attack_draws.npz")
GOLDEN_2 = os.path.join(HERE, "golden", "attack_draws_2.npz")
SEEDS = ((7 << 32) + 11, (1 << 63) + (3 << 32) + 5)       # the second: the key split and the signed conversion see bit 63
DRAWS = (0, 2, 2 ** 32 - 1)
ROWS = (5 + np.arange(8), np.array([2 ** 32 - 1]))


def _collect():
    """{name: array} from the public draw functions alone; integers stay integers, floats keep their own dtype"""
    from awm_amd import attacks as A
    out = {"philox": A.philox4x32_10((np.arange(5, dtype=np.uint64), 0xFFFFFFFE, 2 ** 32 - 1, 2), (11, 0x80000003))}
    for si, seed in enumerate(SEEDS):
        for draw in DRAWS:
            for ri, rows in enumerate(ROWS):
                k = f"s{si}_d{draw}_r{ri}"
                gain, snr, noisy = A.row_parameters(seed, draw, rows, (-6.0, 6.0, 20.0, 40.0, 0.5))
                out[k + "_gain_db"], out[k + "_snr_db"], out[k + "_noisy"] = gain, snr, noisy
                out[k + "_codec_snr_db"] = A.row_snr_db(seed, draw, rows, (10, 30))
                out[k + "_rt60"], out[k + "_drr_db"] = A.row_reverb_params(seed, draw, rows, (0.1, 0.4), (0, 12))
                out[k + "_bank"] = A.row_bank_index(seed, draw, rows, 5)
                out[k + "_warp"] = A.row_warp_params(seed, draw, rows, (0.9, 1.1), (-0.01, 0.02), None, None, 16000)
                out[k + "_warp_flutter"] = A.row_warp_params(seed, draw, rows, (0.8, 1.25), (0.0, 0.0), (0.5, 8.0), (0.0, 0.25), 16000)
                for n in (1, 16000):
                    hi = min(6400, n)
                    spans = A.row_splice_spans(seed, draw, rows, n, max_spans=8, p_span=0.5, len_lo=min(800, hi), len_hi=hi)
                    out[f"{k}_spans_n{n}"] = np.array(spans, dtype=np.int64)           # (rows, 8, {start, L, kind, shift, active})
                row = int(rows[0])
                out[k + "_noise"] = A.normal_noise(seed, draw, row, 9)                 # a ragged last quad
                for K in (1, 33):
                    out[f"{k}_rir_K{K}"] = A.rir_taps(seed, draw, row, 0.3, 6.0, K, 16000)
    return out


def _collect_2():
    """the four draw functions that came after attack_draws.npz was written, at the same seeds, draws and rows"""
    from awm_amd import attacks as A
    out = {}
    for si, seed in enumerate(SEEDS):
        for draw in DRAWS:
            for ri, rows in enumerate(ROWS):
                k = f"s{si}_d{draw}_r{ri}"
                out[k + "_lpc_snr_db"] = A.row_lpc_snr_db(seed, draw, rows, (10, 30))
                out[k + "_reduce_db"] = A.row_reduce_db(seed, draw, rows, (6, 24))
                out[k + "_rate"] = A.row_stretch_rates(seed, draw, rows, (0.9, 1.1))
                out[k + "_semitones"], out[k + "_beta"], out[k + "_pitch_rate"] = A.row_pitch_params(seed, draw, rows, (-1, 1))
    return out


def _same(got, golden):
    with np.load(golden) as want:
        assert sorted(got) == sorted(want.files)
        for k in want.files:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_every_draw_is_what_it_was():
    _same(_collect(), GOLDEN)


def test_the_later_draws_are_what_they_were():
    """attack_draws_2.npz: the package's own output at the last commit before the draws moved into draws.py"""
    _same(_collect_2(), GOLDEN_2)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_attack_draws_cpu.py --write      (writes attack_draws_2.npz alone; attack_draws.npz stays)")
    np.savez_compressed(GOLDEN_2, **_collect_2())
    print(f"wrote {GOLDEN_2}: {os.path.getsize(GOLDEN_2)} bytes")
