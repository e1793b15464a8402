"""Where the wrappers over the C ABI live (no GPU): _host.py (checks and plumbing) <- dsp.py (the waveform ops) <- ops.py (the models'
tape), with every waveform op still reachable as ops.<name>, the public spelling."""
import types

import torch

from awm_amd import dsp, ops

# the public names of the waveform ops as ops.py defined them before dsp.py existed, in its order
WAVEFORM_OPS = [
    "RESAMPLE_LOWPASS_WIDTH", "RESAMPLE_ROLLOFF", "resample_length", "resample_table", "resample_tile_periods", "resample", "resample_add",
    "resample_adjoint_table", "resample_rows", "ResampleRowsFn",
    "BIQUAD_MODES", "BIQUAD_IDENTITY", "biquad_lowpass_coeffs", "biquad_warm", "biquad_plan", "biquad", "PcmCodecFn",
    "DistortFn",
    "MDCT_HOPS", "MDCT_BANDS", "MDCT_GRAD_MODES", "mdct_default_floor_step", "mdct_frames", "mdct_plan", "mdct_kcut", "mdct_codec", "MdctCodecFn",
    "FIR_MAX_TAPS", "fir_rows", "FirRowsFn", "rir_synth",
    "TIME_WARP_MAX_TABLE", "time_warp_table", "time_warp", "TimeWarpFn",
    "WSOLA_MAX_N", "wsola_window", "wsola_frames", "wsola", "WsolaFn",
    "LPC_FRAMES", "LPC_MAX_ORDER", "LPC_GRAD_MODES", "LPC_FLOOR_STEP", "lpc_tables", "lpc_frames", "lpc_codec", "LpcCodecFn",
    "stoi_plan", "stoi",
    "SPLICE_MAX_SPANS", "SPLICE_MAX_N", "label_words", "SpliceFn", "splice", "MaskedBCEFn", "loc_threshold_logit", "loc_counts",
    "CLIP_SCORES_MAX_T", "ClipScores", "clip_scores_plan", "clip_scores", "ClipFeaturesPlan", "clip_features_plan", "clip_features",
]
# the private ones other modules and tests reach through ops
PRIVATE = ["_rate", "_time_warp_table_on", "_wsola_dims", "_lpc_dims", "_lab", "_fir_taps", "_biquad_coeffs", "_stoi_rows"]


def test_all_is_the_list_ops_had():
    assert list(dsp.__all__) == WAVEFORM_OPS and len(set(WAVEFORM_OPS)) == len(WAVEFORM_OPS) == 65


def test_ops_hands_on_the_same_objects():
    for n in WAVEFORM_OPS + PRIVATE:
        assert getattr(ops, n) is getattr(dsp, n), n


def test_where_the_definitions_live():
    for f in (ops.resample, ops.FirRowsFn, ops.clip_features):
        assert f.__module__.endswith(".dsp"), f
    for f in (ops.ResBlockFn, ops.BCEFn):
        assert f.__module__.endswith(".ops"), f


def test_imports_go_one_way():
    import awm_amd
    from awm_amd import _host
    assert awm_amd.dsp is dsp and awm_amd.ops is ops
    for low, high in ((dsp, (ops,)), (_host, (ops, dsp))):
        for name, v in vars(low).items():
            assert not any(v is m for m in high), f"{low.__name__}.{name} is the module {v.__name__}"
            if isinstance(v, types.ModuleType):
                assert not v.__name__.startswith("awm_amd.") or v is _host, f"{low.__name__} imports {v.__name__}"
    for n in ("_stream", "_p", "_chk", "_chk_int", "_chk_positive", "_seed64", "_f32"):     # one definition, bound in both namespaces
        assert getattr(ops, n) is getattr(dsp, n) is getattr(_host, n), n


def test_one_cache_of_device_copies():
    made = []

    def make():
        made.append(1)
        return torch.arange(3.0)

    key = ("test_dsp_layout", 1)
    try:
        a = dsp._on_device(key, torch.device("cpu"), make)
        b = dsp._on_device(key, torch.device("cpu"), make)
        assert a is b and made == [1] and torch.equal(a, torch.arange(3.0))
        pair = dsp._on_device(key + ("pair",), "cpu", lambda: (torch.zeros(2), torch.ones(2, dtype=torch.int32)))
        assert isinstance(pair, tuple) and pair[1].dtype == torch.int32 and pair is dsp._on_device(key + ("pair",), torch.device("cpu"), make)
        assert made == [1]
        # the families' own entries go through it: one device copy per (table, device), whichever spelling of the device
        w = dsp._wsola_window_on(64, torch.device("cpu"))
        assert w is dsp._wsola_window_on(64, "cpu") and torch.equal(w, dsp.wsola_window(64))
        assert dsp._time_warp_table_on(4, 64, "cpu") is ops._time_warp_table_on(4, 64, torch.device("cpu"))
        lag, expand = dsp._lpc_tables_on(8, 16000, "cpu")
        assert torch.equal(lag, dsp.lpc_tables(8, 16000)[0]) and torch.equal(expand, dsp.lpc_tables(8, 16000)[1])
        fwd, adj = dsp.resample_table(3, 2), dsp.resample_adjoint_table(3, 2)           # a rate pair and its adjoint: two entries
        taps, first = dsp._resample_on(fwd, (3, 2), "cpu")
        taps_a, first_a = dsp._resample_on(adj, (3, 2, "adjoint"), "cpu")
        assert torch.equal(taps, fwd["taps"]) and torch.equal(first, fwd["first"])
        assert torch.equal(taps_a, adj["taps"]) and torch.equal(first_a, adj["first"]) and taps_a.shape != taps.shape
    finally:
        for k in [k for k in dsp._ON_DEVICE if k[0][0] == "test_dsp_layout"]:
            del dsp._ON_DEVICE[k]
