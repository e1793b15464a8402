"""What the GPU test files share that is no yardstick: the two fixtures, the main16 models at the reference's initial state, and a few
small helpers.  A test file takes the fixtures with `from gpu_support import awm, dev  # noqa: F401` and the rest by name."""
import math

import numpy as np
import pytest
import torch

from oracle import recipes as R


@pytest.fixture(scope="module")
def awm():
    import awm_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    awm_amd.lib.load()
    return awm_amd


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def reference_models(awm, dev, perturb_bn=True):
    """(Generator(16), Detector(16)) on `dev` at the reference's seeded initial state, in training mode as constructed; perturb_bn moves
    the BatchNorm statistics and affine parameters off their trivial values"""
    gsd, dsd = R.reference_layout_init()
    if perturb_bn:
        R.perturb_bn_(gsd, R.BN_SEED_G)
        R.perturb_bn_(dsd, R.BN_SEED_D)
    G, D = awm.Generator(16), awm.Detector(16)
    G.load_state_dict(gsd)
    D.load_state_dict(dsd)
    return G.to(dev), D.to(dev)


def rel_err(a, ref):
    """max |a - ref| relative to max |ref|, in float64"""
    a, ref = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-30))


def check(a, ref, tol, what=""):
    assert tuple(a.shape) == tuple(ref.shape), f"{what}: shape {tuple(a.shape)} vs {tuple(ref.shape)}"
    e = rel_err(a, ref)
    print(f"{what}: rel err {e:.3e}")
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol}"


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def bits(t):
    """the float32 tensor's bit patterns, for comparisons that -0.0 and NaN must not pass"""
    return t.contiguous().view(torch.int32)


CANARY = 8                         # untouched elements on either side of a Guarded buffer
PATTERN = 0x5A5A5A5A
INVALID = 1                        # hipErrorInvalidValue


class Guarded:
    """n elements with CANARY more on either side: NaN around floats, a bit pattern around integers.  `t` is the inner view (16-byte
    aligned: CANARY * 4 bytes in); intact() is true while the surround, and with whole=True everything, holds what it was given.
    Without `init` the inner elements hold the fill too: an output element the kernel never writes stays NaN."""

    def __init__(self, dev, n, init=None, dtype=torch.float32):
        fill = float("nan") if dtype == torch.float32 else (PATTERN if dtype == torch.int32 else PATTERN << 32 | PATTERN)
        self.buf = torch.full((n + 2 * CANARY,), fill, dtype=dtype, device=dev)
        self.t = self.buf[CANARY:CANARY + n]
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(dev).reshape(-1))
        self.before = self.buf.clone()

    def intact(self, whole=False):
        a, b = self.buf, self.before
        if a.dtype == torch.float32:
            a, b = bits(a), bits(b)
        n, C = self.t.numel(), CANARY
        return bool(torch.equal(a, b)) if whole else bool(torch.equal(a[:C], b[:C]) and torch.equal(a[C + n:], b[C + n:]))

    def np(self, shape=None):
        a = self.t.cpu().numpy()
        return a if shape is None else a.reshape(shape)


def invalid(call, *outputs):
    """the call returns hipErrorInvalidValue and writes nothing"""
    with pytest.raises(RuntimeError, match=f"hipError {INVALID}$"):
        call()
    torch.cuda.synchronize()
    for g in outputs:
        assert g.intact(whole=True), "an invalid call wrote to an output"


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def p(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


def same(a, b):
    """equality through dicts, sequences, tensors and arrays; NaN equals NaN"""
    if isinstance(a, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b))


def _spy(monkeypatch, lib, names):
    """wrap lib.<name> for every name so that calls are counted: {name: calls}"""
    counts = {}
    for name in names:
        real = getattr(lib, name)

        def spy(*a, _real=real, _name=name):
            counts[_name] = counts.get(_name, 0) + 1
            return _real(*a)
        monkeypatch.setattr(lib, name, spy)
    return counts
