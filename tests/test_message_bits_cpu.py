"""Generator(bits) / Detector(bits) at payload widths other than 0 and 16: parameter names, shapes, dtypes and initial
values against the oracle's reference-layout init (py/main16.py:129-147, 171-181).  No GPU needed."""
import pytest
import torch

from oracle import recipes as R


@pytest.mark.parametrize("bits", [1, 8, 20])
def test_constructors_match_reference_layout(bits):
    import awm_amd
    torch.manual_seed(R.WEIGHT_SEED)
    G, D = awm_amd.Generator(bits), awm_amd.Detector(bits)
    gsd, dsd = R.reference_layout_init(bits)
    for mod, ref in ((G, gsd), (D, dsd)):
        sd = mod.state_dict()
        assert list(sd.keys()) == list(ref.keys())
        for k, v in ref.items():
            assert sd[k].shape == v.shape and sd[k].dtype == v.dtype, k
            assert torch.equal(sd[k], v), k
    assert G.embedding.weight.shape == (2 ** bits, 64)
    assert D.model[3].weight.shape == (1 + bits, 64, 1)


@pytest.mark.parametrize("bits", [32, 63])
def test_wide_detector_layout(bits):
    import awm_amd
    D = awm_amd.Detector(bits)
    _, dsd = R.reference_layout_init(0)
    keys = list(D.state_dict().keys())
    assert keys == list(dsd.keys())
    assert D.model[3].weight.shape == (1 + bits, 64, 1)
    assert D.model[3].bias.shape == (1 + bits,)
