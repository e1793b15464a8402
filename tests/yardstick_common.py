"""What several float64 yardsticks need and none of them owns: the unit roundoff of float32, the summation bound built on it, one
float32 ulp of a float64 result, and the comparison every derived tolerance ends in.  Numpy alone; nothing from the package."""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    """n u / (1 - n u): n roundings of relative size u, in any order (Higham, Accuracy and Stability, ch. 3)"""
    return n * U / (1 - n * U)


def ulp32(v):
    """the spacing of float32 at |v|, as float64"""
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def assert_within(y, ref, bound, what):
    """|y - ref| <= bound at every sample; the worst sample is named.  Against a one-dimensional reference y is read flat, so a (1, L)
    tensor of the package stands against an (L,) yardstick; any other reference needs y in its own shape.  Nothing to compare passes."""
    y = np.asarray(y, dtype=np.float64)
    if ref.ndim == 1:
        y = y.reshape(-1)
    assert y.shape == ref.shape, f"{what}: {y.shape} vs {ref.shape}"
    if y.size:
        err = np.abs(y - ref)
        worst = np.unravel_index(int(np.argmax(err - bound)), err.shape)
        print(f"{what}: max err {err.max():.3e}, max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound), f"{what}: sample {worst}: err {err[worst]:.3e} > bound {bound[worst]:.3e}"
