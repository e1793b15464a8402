"""The noise-suppression attack without a GPU: the yardstick of tests/suppress_yardstick.py against the definition's own properties
(identity at reduce_db = 0, the adjoint identity, silence, the unbiased noise estimate), the draw (word o3 of the warp_phase counter), the
CPU path of attacks.NoiseSuppress and suppress.noise_suppress against the yardstick, the draws' bookkeeping, refusals, and the C boundary."""
import importlib
import os

import numpy as np
import pytest
import torch

import draw_yardstick as D
import suppress_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "audio-watermarking-deep-learning-watermarks-for-authenticating-speech_amd")


def S():
    return importlib.import_module("awm_amd.suppress")


# ------------------------------------------------------------------------------------------ the yardstick against the definition
@pytest.mark.parametrize("n", [1, 255, 256, 257, 700, 16000])
def test_identity_at_reduce_db_zero(n):
    x = Y.case(n).astype(np.float64)
    for i in range(3):
        y, G, N = Y.model(x[i], 0.0)
        assert (G == 1.0).all() and G.shape == (Y.frame_count(n), 257) and N.shape == (257,)
        assert np.abs(y - x[i]).max() <= 1e-12
    assert float(Y.window() @ Y.window()) == pytest.approx(256.0, abs=1e-9)
    assert np.abs(Y.window()[:256] ** 2 + Y.window()[256:] ** 2 - 1.0).max() < 1e-15, "w^2 sums to 1 at 50 % overlap"


@pytest.mark.parametrize("n", [257, 700, 4000])
def test_adjoint_identity_with_the_gains_held(n):
    x = Y.case(n).astype(np.float64)
    rng = np.random.default_rng(n)
    for i in range(3):
        u, v = rng.standard_normal(n), rng.standard_normal(n)
        Au, Av = Y.model(x[i], 20.0, src=u)[0], Y.model(x[i], 20.0, src=v)[0]
        a, b = float(Au @ v), float(u @ Av)
        assert abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (i, a, b)
        assert np.abs(Y.model(x[i], 20.0)[1] - Y.model(x[i], 20.0, src=u)[1]).max() == 0.0, "the gains come from x alone"


def test_zeros_in_zeros_out():
    for twin in (False, True):
        y, G, N = Y.model(np.zeros(700), 18.0, twin=twin)
        assert not y.any() and np.isfinite(G).all() and np.isfinite(N).all() and (N > 0).all()
        assert (G[1:] == G.dtype.type(10.0) ** G.dtype.type(-0.9)).all()
    y, G, N = Y.model(np.array([0.1, np.nan, 0.2]), 18.0)
    assert np.isnan(y).all() and np.isnan(G).all() and np.isnan(N).all()


def test_noise_estimate_is_unbiased_on_gaussian_noise():
    sigma, n = 0.05, 16000 * 8
    x = sigma * np.random.default_rng(3).standard_normal(n)
    N = Y.model(x, 12.0)[2]
    true = sigma ** 2 * 256.0                                                      # sigma^2 sum w^2
    inner = N[1:256]                                                               # the two real-valued bins are chi-squared with ONE degree
    assert abs(inner.mean() / true - 1.0) < 0.03, inner.mean() / true
    assert np.abs(inner / true - 1.0).max() < 0.25


def test_clip_of_reduce_db_and_the_twin():
    x = Y.case(700)[0]
    assert Y.clip_db(float("nan")) == 0.0 and Y.clip_db(75.0) == 60.0 and Y.clip_db(-3.0) == 0.0
    for a, b in ((float("nan"), 0.0), (75.0, 60.0), (-1.0, 0.0)):
        assert all(np.array_equal(u, v) for u, v in zip(Y.model(x, a), Y.model(x, b)))
    fy, fG, fN = Y.floors(700)
    print(f"float32 floors at n = 700: y {fy:.2e}, G {fG:.2e}, N / max N {fN:.2e}")
    assert all(v.dtype == np.float32 for v in Y.ref(700, twin=True)[0]) and 0 < fy < 1e-5 and 0 < fG < 1e-3 and 0 < fN < 1e-5


# ------------------------------------------------------------------------------------------ draws and counters
def test_draw_is_word_o3_of_the_warp_phase_counter():
    from awm_amd import attacks
    seed, draw, rows = (5 << 32) + 9, 3, np.arange(7, 40)
    r = attacks.row_reduce_db(seed, draw, rows, (6, 24))
    o = D.philox4x32_10((*D.WARP_PHASE, rows, draw), D.key_of(seed))
    assert r.dtype == np.float32 and r.shape == (33,) and np.array_equal(r, D.affine32((6, 24), D.unit(o[3])))
    assert (r >= 6).all() and (r <= 24).all() and len(set(r)) == 33
    assert not np.array_equal(r, attacks.row_reduce_db(seed, draw + 1, rows, (6, 24)))
    assert not np.array_equal(r, attacks.row_reduce_db(seed + 1, draw, rows, (6, 24)))
    assert (attacks.row_reduce_db(seed, draw, rows, (18, 18)) == np.float32(18)).all()
    # its three neighbours keep their words
    assert np.array_equal(attacks.row_stretch_rates(seed, draw, rows, (0.8, 1.25)), D.affine32((0.8, 1.25), D.unit(o[1])))
    assert np.array_equal(attacks.row_pitch_params(seed, draw, rows, (-3, 4))[0], D.affine32((-3, 4), D.unit(o[2])))


def test_families_are_unchanged():
    from awm_amd import attacks, ops
    fixed = {name: f for name, f in attacks.FAMILIES.items() if f[0] is not None}
    assert fixed == D.FAMILIES and len(attacks.FAMILIES) == 6 + 2 * ops.SPLICE_MAX_SPANS
    assert list(attacks.FAMILIES)[:6] == ["sample", "rir_tap", "param", "param2", "warp", "warp_phase"]


# ------------------------------------------------------------------------------------------ the package's host path
@pytest.mark.parametrize("n", [1, 257, 700, 4000])
def test_host_path_matches_the_yardstick(n):
    import awm_amd
    x = torch.from_numpy(np.array(Y.case(n)))
    rd = torch.tensor(Y.REDUCE_DB)
    y, G, N = awm_amd.noise_suppress(x, rd, gains_out=True)
    r64 = Y.ref(n)
    assert y.dtype == G.dtype == N.dtype == torch.float32 and tuple(G.shape) == (3, Y.frame_count(n), 257) and tuple(N.shape) == (3, 257)
    for i in range(3):
        ey, eG, eN = Y.errors((y[i].numpy(), G[i].numpy(), N[i].numpy()), r64[i])
        assert ey <= 2e-7 and eG <= 1e-7 and eN <= 1e-7, (i, ey, eG, eN)           # float32 storage of a float64 result
    dy = torch.from_numpy(np.array(Y.cotangent(n)))
    yb = awm_amd.noise_suppress(x, rd, src=dy)
    prof = torch.from_numpy(np.array(Y.profile(n)))
    yp, Gp, Np = awm_amd.noise_suppress(x, rd, noise_psd=prof, gains_out=True)
    for i in range(3):
        assert Y.errors((yb[i].numpy(), G[i].numpy(), N[i].numpy()), Y.ref(n, "backward")[i])[0] <= 2e-7
        ey, eG, eN = Y.errors((yp[i].numpy(), Gp[i].numpy(), Np[i].numpy()), Y.ref(n, "profile")[i])
        assert ey <= 2e-7 and eG <= 1e-7 and eN == 0.0
    # the module is the functional at its draws
    m = awm_amd.NoiseSuppress((6, 24), seed=4)
    got = m(x)
    assert torch.equal(got, awm_amd.noise_suppress(x, m.last_reduce_db))
    assert np.array_equal(m.last_reduce_db.numpy(), awm_amd.attacks.row_reduce_db(4, 0, np.arange(3), (6, 24)))


def test_shapes_and_edge_rows_on_the_host():
    import awm_amd
    x = torch.from_numpy(np.array(Y.case(700)))
    want = awm_amd.noise_suppress(x, 18.0)
    for a, shape in ((x[:, None], (3, 1, 700)), (x, (3, 700)), (x[2], (700,))):
        got = awm_amd.NoiseSuppress(18)(a)
        assert tuple(got.shape) == shape and got.dtype == torch.float32
        assert torch.equal(got.reshape(-1, 700), want if len(shape) > 1 else want[2:3])
        assert tuple(awm_amd.noise_suppress(a, 18.0).shape) == shape
    assert float((awm_amd.noise_suppress(x, 0.0) - x).abs().max()) <= 6e-8, "reduce_db = 0 hands the input on, to float32 storage"
    z = torch.zeros(2, 700)
    y, G, N = awm_amd.noise_suppress(z, 18.0, gains_out=True)
    assert not y.any() and bool(torch.isfinite(G).all())
    bad = x.clone()
    bad[1, 300] = float("nan")
    yb, Gb, Nb = awm_amd.noise_suppress(bad, 18.0, gains_out=True)
    assert bool(torch.isnan(yb[1]).all()) and bool(torch.isnan(Gb[1]).all()) and bool(torch.isnan(Nb[1]).all())
    assert torch.equal(yb[0], want[0]) and torch.equal(yb[2], want[2])
    for a, b in ((float("nan"), 0.0), (75.0, 60.0)):
        assert torch.equal(awm_amd.noise_suppress(x, a), awm_amd.noise_suppress(x, b))


def test_inside_sequential_with_distortion_and_the_pcm_codec():
    import awm_amd
    x = torch.from_numpy(np.array(Y.case(2000)))[:, None]
    chain = torch.nn.Sequential(awm_amd.Distortion(gain_db=0, snr_db=30, seed=1), awm_amd.NoiseSuppress(12, seed=2), awm_amd.PcmCodec())
    y = chain(x)
    assert tuple(y.shape) == (3, 1, 2000) and bool(torch.isfinite(y).all())
    step = awm_amd.PcmCodec()(awm_amd.NoiseSuppress(12, seed=2)(awm_amd.Distortion(gain_db=0, snr_db=30, seed=1)(x)))
    assert torch.equal(y, step)


def test_draws_rewind_and_follow_row0():
    import awm_amd
    x = torch.from_numpy(np.array(Y.case(700)))
    m = awm_amd.NoiseSuppress((6, 24), seed=11)
    a, da = m(x), m.last_reduce_db
    b, db = m(x), m.last_reduce_db
    assert m.draw == 2 and not torch.equal(da, db) and not torch.equal(a, b)
    m.reset()
    assert torch.equal(m(x), a) and torch.equal(m.last_reduce_db, da)
    m.reset(1)
    assert torch.equal(m(x), b)
    m.reset()
    head = m(x[:2])
    m.reset()
    tail = m(x[2:], row0=2)
    assert torch.equal(torch.cat([head, tail]), a), "a batch cut into pieces draws what the whole batch would"
    m.reset(5)
    for bad_x, kw in ((torch.zeros(0), {}), (x, {"row0": -1}), (x, {"row0": 2 ** 32}), (torch.zeros(2, 2, 2, 4), {})):
        with pytest.raises(ValueError):
            m(bad_x, **kw)
    with pytest.raises(TypeError):
        m(x.numpy())
    mp = awm_amd.NoiseSuppress(12, noise_psd=torch.ones(2, 257))
    with pytest.raises(ValueError):
        mp(x)                                                                      # a profile for two rows, three rows
    assert m.draw == 5 and mp.draw == 0, "a call that raises consumes no draw"
    assert "reduce_db=(6.0, 24.0)" in repr(m) and "seed=11" in repr(m) and "alpha=0.98" in repr(m)


def test_bad_arguments_raise_value_error():
    import awm_amd
    for kw in (dict(reduce_db=(24, 6)), dict(reduce_db=-1), dict(reduce_db=61), dict(reduce_db=float("nan")), dict(reduce_db="6"),
               dict(reduce_db=(1, 2, 3)), dict(alpha=1.0), dict(alpha=-0.1), dict(alpha=float("nan")), dict(alpha=True), dict(over=0.0),
               dict(over=float("inf")), dict(over=-1.0), dict(seed=1.5), dict(noise_psd=torch.ones(256)), dict(noise_psd=[1.0] * 257),
               dict(noise_psd=-torch.ones(257)), dict(noise_psd=torch.full((257,), float("nan")))):
        with pytest.raises(ValueError):
            awm_amd.NoiseSuppress(**kw)
    x = torch.zeros(2, 700)
    for args, kw in (((x, torch.zeros(3)), {}), ((x, "6"), {}), ((x, True), {}), ((x.double(), 6.0), {}), ((torch.zeros(2, 2, 700), 6.0), {}),
                     ((torch.zeros(2, 0), 6.0), {}), ((x, 6.0), dict(src=torch.zeros(2, 699))), ((x, 6.0), dict(alpha=1.0)),
                     ((x, 6.0), dict(over=0.0)), ((x, 6.0), dict(noise_psd=torch.ones(3, 257))), ((x, 6.0), dict(noise_psd=-torch.ones(257)))):
        with pytest.raises(ValueError):
            awm_amd.noise_suppress(*args, **kw)
    with pytest.raises(TypeError):
        awm_amd.noise_suppress(x.numpy(), 6.0)
    for rows, n in ((0, 100), (1, 0), (1, 2 ** 34 + 1), (2 ** 20, 2 ** 30), (1.5, 10), (True, 10)):
        with pytest.raises(ValueError):
            S().suppress_plan(rows, n)


# ------------------------------------------------------------------------------------------ the C boundary
def test_entry_points_are_declared_exported_and_built():
    from awm_amd import _lib
    protos = _lib.parse_header()
    assert protos["wm_noise_suppress_plan"] == [("long long", "rows"), ("long long", "n"), ("long long*", "frames"),
                                                ("long long*", "scratch_bytes"), ("wm_stream_t", "stream")]
    assert protos["wm_noise_suppress"] == [("const float*", "x"), ("const float*", "src"), ("const float*", "noise_in"),
                                           ("const float*", "reduce_db"), ("float*", "y"), ("float*", "gain_out"), ("float*", "noise_out"),
                                           ("void*", "scratch"), ("long long", "rows"), ("long long", "n"), ("float", "alpha"),
                                           ("float", "over"), ("wm_stream_t", "stream")]
    assert os.path.isfile(os.path.join(PKG, "csrc", "noise_suppress.hip"))
    text = open(os.path.join(PKG, "csrc", "noise_suppress.hip")).read()
    for name in ("wm_noise_suppress_plan", "wm_noise_suppress"):
        assert f"int {name}(" in text
    assert "fft_dif<9>" in text and "atomic" not in text.lower().replace("no atomics", "")
    units = open(os.path.join(PKG, "csrc", "build.sh")).read().split("for f in ")[1].split(";")[0].split()
    assert "noise_suppress" in units and units.count("noise_suppress") == 1
    dll = _lib.lib.load()
    for name in ("wm_noise_suppress_plan", "wm_noise_suppress"):
        assert hasattr(dll, name)
    import awm_amd
    for name in ("NoiseSuppress", "noise_suppress"):
        assert name in awm_amd.__all__ and hasattr(awm_amd, name)
    assert list(awm_amd.__all__[-3:]) == ["masking", "MaskingLoss", "nmr"]
    assert awm_amd.NoiseSuppress is awm_amd.attacks.NoiseSuppress and issubclass(awm_amd.NoiseSuppress, awm_amd.attacks._RowDraws)


def test_plan_is_a_host_query():
    for rows, n in ((1, 1), (3, 255), (3, 256), (3, 257), (512, 16000), (1, 57_600_000)):
        frames, need = S().suppress_plan(rows, n)
        chunks = -(-frames // 16)
        assert frames == Y.frame_count(n) == S().suppress_frames(n)
        assert need == rows * (frames * 257 * 4 + chunks * 257 * 8 + chunks * 4)
    assert S().suppress_plan(1, 57_600_000)[0] == 225_001                          # an hour in one row
    assert S().suppress_plan(1, 1)[0] == 2 and S().suppress_plan(1, 256)[0] == 2 and S().suppress_plan(1, 257)[0] == 3
