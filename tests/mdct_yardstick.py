"""The float64 yardstick of the transform codec (wm_mdct_codec / attacks.TransformCodec), written from the definition in include/wm_hip.h
with numpy alone -- nothing from the package -- and shared by tests/test_mdct_codec_cpu.py and tests/test_gpu_mdct_codec.py.

codec(x, ..., dtype=np.float64) is the definition, dense: the (M, 2M) cosine matrix, frames cut from the zero-extended row, the per-band
step, rint, the transposed matrix, overlap-add.  `codes=` replaces its own rounding decisions (Xq = codes * step, the step still its own);
`mask=` zeroes the coefficients where it holds 0.  dtype=np.float32 is the same text with every array in float32: the "float32 restatement"
whose distance from float64 sizes the tolerances of the GPU tests (E32) and the near-tie set of the codes (h = 8 max|r32 - r64|)."""
import numpy as np

KCUT = {128: 112, 256: 224, 512: 448}            # 7 kHz at 16 kHz: a multiple of every band size
# the issue's shapes, then hop 512 (its own LDS size), then a row of 94 hops: two 64-frame workgroups at hop 256
BAND = 8
SNR_DB = (10.0, 20.0, 30.0)                       # row r gets SNR_DB[r % 3]
NS = lambda M: (1, M - 1, M, M + 1, 4 * M + 3, 16000)
GPU_CASES = [(rows, M, n) for rows in (1, 3) for M in (128, 256) for n in NS(M)] + [(2, 512, n) for n in (511, 4 * 512 + 3, 16000)] + [(1, 256, 24059)]


def default_floor_step(M):
    return 2.0 ** -15 * np.sqrt(M / 2.0)


def signal(rows, n):
    """the issue's input: 0.1 * normal + 0.2 * sin(2 pi 440 t / 16000), float32, from default_rng(0)"""
    t = np.arange(n)
    return (0.1 * np.random.default_rng(0).standard_normal((rows, n)) + 0.2 * np.sin(2 * np.pi * 440 * t / 16000)).astype(np.float32)


def degenerate(n):
    """(3, n): an all-zero row, a row at amplitude 1e-7 (everything under the floor step), a pure 440 Hz tone (most bands at the floor)"""
    x = signal(3, n)
    x[0] = 0
    x[1] *= np.float32(1e-6)                                                      # 0.1 * normal + 0.2 * sin  ->  about 1e-7
    x[2] = (0.2 * np.sin(2 * np.pi * 440 * np.arange(n) / 16000)).astype(np.float32)
    return x


def snr_rows(rows):
    return np.array([SNR_DB[r % 3] for r in range(rows)], dtype=np.float32)


def basis(M, dtype=np.float64):
    """window w (2M,) and C[k][j] = cos(pi/M (j + 1/2 + M/2)(k + 1/2)), evaluated in float64 and rounded once to dtype"""
    j, k = np.arange(2 * M, dtype=np.float64), np.arange(M, dtype=np.float64)
    w = np.sin(np.pi * (j + 0.5) / (2 * M))
    return w.astype(dtype), np.cos(np.pi / M * np.outer(k + 0.5, j + 0.5 + M / 2)).astype(dtype)


def codec(x, M, band, kcut, snr_db, floor_step, quantise=True, codes=None, mask=None, dtype=np.float64):
    """x (rows, n) -> dict(y (rows, n), X (rows, F, M) after cut and mask, step (rows, F, M), r = X / step, codes int64, Xq), all in dtype"""
    x = np.asarray(x, dtype=dtype)
    rows, n = x.shape
    nb = -(-n // M)
    F = nb + 1
    w, C = basis(M, dtype)
    xp = np.zeros((rows, (F + 1) * M), dtype=dtype)
    xp[:, M:M + n] = x                                                            # frame f: samples (f-1)M .. (f+1)M - 1
    fr = np.stack([xp[:, f * M:(f + 2) * M] for f in range(F)], axis=1)           # (rows, F, 2M)
    X = (fr * w) @ C.T                                                            # (rows, F, M)
    X[:, :, kcut:] = 0
    if mask is not None:
        X = np.where(np.asarray(mask) != 0, X, dtype(0))
    P = (X.reshape(rows, F, M // band, band) ** 2).mean(axis=3)
    scale = (dtype(10) ** (-np.asarray(snr_db, dtype=dtype) / dtype(20))).reshape(rows, 1, 1)
    step = np.repeat(np.maximum(np.sqrt(dtype(12) * P) * scale, dtype(floor_step)), band, axis=2)
    r = X / step
    q = np.rint(r).astype(np.int64) if codes is None else np.asarray(codes, dtype=np.int64)
    Xq = (q.astype(dtype) * step) if quantise else X
    yf = dtype(2.0 / M) * w * (Xq @ C)                                            # (rows, F, 2M)
    out = np.zeros((rows, (F + 1) * M), dtype=dtype)
    for f in range(F):
        out[:, f * M:(f + 2) * M] += yf[:, f]
    return dict(y=out[:, M:M + n], X=X, step=step, r=r, codes=q, Xq=Xq)


def near_tie(x, M, band, kcut, snr_db, floor_step):
    """(tie, share, r64, codes64): tie marks the coefficients whose r64 = X / step lies within h = 8 max|r32 - r64| of a half-integer"""
    a = codec(x, M, band, kcut, snr_db, floor_step)
    b = codec(x, M, band, kcut, snr_db, floor_step, dtype=np.float32)
    h = 8.0 * float(np.abs(b["r"].astype(np.float64) - a["r"]).max())
    tie = np.abs(np.abs(a["r"] - np.floor(a["r"])) - 0.5) <= h
    return tie, float(tie.mean()), a, b, h


def e32(x, M, band, kcut, mask=None):
    """the largest error of the float32 restatement of the linear map (quantiser off) against float64 on this input, and the float64 result"""
    a = codec(x, M, band, kcut, np.zeros(len(x)), 1.0, quantise=False, mask=mask)
    b = codec(x, M, band, kcut, np.zeros(len(x)), 1.0, quantise=False, mask=mask, dtype=np.float32)
    return float(np.abs(b["y"].astype(np.float64) - a["y"]).max()), a
