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
