"""GPU parity of the main14b_2 variant (BASELINE config 5), forward path: generic conv kernel vs torch CPU ops on
awkward shapes, whole Generator / Detector vs the reference fixtures (tests/golden/main14b2_golden.npz) and the oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import wm_oracle as O
from oracle import wm_oracle_14b2 as O2

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def M():
    import awm_amd
    awm_amd.lib.load()
    from awm_amd import main14b_2
    return main14b_2


@pytest.fixture(scope="module")
def g2():
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "main14b2_golden.npz"))


def rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-30))


def check_elementwise(a, ref, what="", rtol=1e-4, atol_of_max=1e-6):
    """north_star's 1e-4 rtol, element by element: |a - ref| <= rtol*|ref| + atol_of_max*max|ref| (the absolute term is the fp32
    round-off floor of a value formed by summing terms of magnitude max|ref|) -- same bar as tests/test_gpu_parity.py"""
    assert a.shape == ref.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(ref.shape)}"
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    excess = (a - ref).abs() - (rtol * ref.abs() + atol_of_max * float(ref.abs().max()))
    worst = float(excess.max())
    assert worst <= 0.0, (f"{what}: {int((excess > 0).sum())} of {a.numel()} elements outside rtol {rtol} + {atol_of_max}*max; "
                          f"worst excess {worst:.3e} at ref = {float(ref.flatten()[int(excess.argmax())]):.3e}")


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("cin,cout,k,stride,pad,L", [(1, 32, 7, 1, 3, 1000), (32, 64, 3, 2, 1, 1000), (64, 128, 3, 4, 1, 501),
                                                     (128, 256, 3, 5, 1, 400), (256, 512, 3, 8, 1, 399), (32, 64, 1, 2, 0, 1000),
                                                     (8, 1, 7, 1, 3, 700), (32, 17, 7, 1, 3, 333), (512, 256, 1, 1, 0, 50)])
def test_gconv_matches_conv1d(M, cin, cout, k, stride, pad, L):
    dev = torch.device("cuda:0")
    x, w, b = rnd(2, cin, L, seed=1), rnd(cout, cin, k, seed=2, scale=0.1), rnd(cout, seed=3)
    ref = F.elu(F.conv1d(x, w, b, stride=stride, padding=pad))
    with torch.no_grad():
        y = M._gconv(x.to(dev), w.to(dev), b.to(dev), stride, pad, act=1)
    assert rel(y, ref) <= TOL
    res = rnd(*ref.shape, seed=4)
    ref2 = F.conv1d(x, w, b, stride=stride, padding=pad) + res
    with torch.no_grad():
        y2 = M._gconv(x.to(dev), w.to(dev), b.to(dev), stride, pad, act=0, res=res.to(dev))
    assert rel(y2, ref2) <= TOL


@pytest.mark.parametrize("cin,cout,st,L", [(128, 64, 8, 50), (64, 32, 5, 400), (32, 16, 4, 2001), (16, 8, 2, 1000), (512, 256, 8, 50)])
def test_gconvT_matches_conv_transpose1d(M, cin, cout, st, L):
    dev = torch.device("cuda:0")
    x, w, b = rnd(2, cin, L, seed=5), rnd(cin, cout, 2 * st, seed=6, scale=0.1), rnd(cout, seed=7)
    ref = F.conv_transpose1d(x, w, b, stride=st, padding=st // 2)
    with torch.no_grad():
        y = M._gconvT(x.to(dev), w.to(dev), b.to(dev), st)
    assert rel(y, ref) <= TOL


@pytest.mark.parametrize("cin,cout,k,stride,pad,L", [(128, 128, 3, 1, 1, 2001), (256, 256, 3, 1, 1, 400), (64, 128, 3, 4, 1, 2001),
                                                     (32, 64, 3, 2, 1, 1000), (512, 256, 1, 1, 0, 50), (256, 128, 7, 1, 3, 50),
                                                     (128, 256, 1, 5, 0, 2001), (16, 8, 3, 1, 1, 4000)])
@pytest.mark.parametrize("gscale", [1.0, 1e-8, 3e3])
def test_gconv_f16_split_is_fp32_grade(M, cin, cout, k, stride, pad, L, gscale):
    """the generic convolution on the f16 two-piece split (wm_gconv_h: three products per product; weight image at the fixed scale 2^8,
    as the package packs every image (wm_gconv_pack_h_conv, wm_gconv_pack_h with scratch = NULL; the max-|w| scale of wm_gconv_pack_h is
    test_gpu_main14b2_kernels.py::test_gconv_pack_h_scaled_route's), a gradient input scaled from max |g| by wm_gscale_absmax) beside
    the native fp32-MFMA build (wm_gconv) on the same inputs,
    both against fp64: forward with ELU, and the data gradient for upstream gradient magnitudes 1e-8 ... 3e3 (strided layers take the
    transposed / pixel-shuffled route).  Error relative to the result's max below 1e-6 and within 3x of the fp32 build's + 2e-7."""
    dev = torch.device("cuda:0")
    x, w, b = rnd(2, cin, L, seed=11), rnd(cout, cin, k, seed=12, scale=0.1), rnd(cout, seed=13)
    Lout = (L + 2 * pad - k) // stride + 1
    g = rnd(2, cout, Lout, seed=14) * gscale
    xr, wr = x.double().requires_grad_(), w.double()
    yr = F.elu(F.conv1d(xr, wr, b.double(), stride=stride, padding=pad))
    zr = F.conv1d(xr, wr, b.double(), stride=stride, padding=pad)
    (dxr,) = torch.autograd.grad(zr, xr, g.double())
    outs = []
    for h in (False, True):
        with torch.no_grad(), M.ops.switches(gconv_f16x3=h):
            y = M._gconv(x.to(dev), w.to(dev), b.to(dev), stride, pad, act=1) if gscale == 1.0 else None
            dx = M._conv_dgrad(g.to(dev), w.to(dev), stride, pad, L)
        outs.append((y, dx))
    for name, a, h_, r in (("y", outs[0][0], outs[1][0], yr), ("dx", outs[0][1], outs[1][1], dxr)):
        if a is None:
            continue
        e_n, e_h = rel(a, r.detach().float()), rel(h_, r.detach().float())
        e_n, e_h = float((a.double().cpu() - r.detach()).abs().max() / r.detach().abs().max()), float((h_.double().cpu() - r.detach()).abs().max() / r.detach().abs().max())
        print(f"{cin}>{cout} k{k} s{stride} g x {gscale:g} {name}: fp32 mfma {e_n:.2e} f16 split {e_h:.2e}")
        assert e_h < 1e-6 and e_h < 3 * e_n + 2e-7, (name, e_n, e_h)


@pytest.mark.parametrize("hd", [256, 32])
def test_main14b2_forward_golden(M, g2, hd):
    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    G, D = M.Generator(hidden_dim=hd), M.Detector()
    gsd = {k: v.detach().clone() for k, v in G.state_dict().items()}
    dsd = {k: v.detach().clone() for k, v in D.state_dict().items()}
    G.to(dev).eval(); D.to(dev).eval()
    s = O.synthetic_clips(2, seed=1234)
    msg = torch.from_numpy(g2["message"])
    with torch.no_grad():
        d = G(s.to(dev), msg.to(dev))
        assert d.shape == (2, 1, 16000)
        assert rel(d, torch.from_numpy(g2[f"hd{hd}_delta"])) <= TOL
        # element by element against the reference fixtures: the fp32 CPU reference itself sits ~1e-6 of max away from an fp64 run
        # through these ~50 layers (no normalisation layer re-centres the error), hence the absolute floor
        check_elementwise(d, torch.from_numpy(g2[f"hd{hd}_delta"]), f"hd{hd} delta (element-wise)", atol_of_max=5e-6)
        d0 = G(s.to(dev))
        assert rel(d0[..., ::97], torch.from_numpy(g2[f"hd{hd}_delta_nomsg_sub"])) <= TOL
        check_elementwise(d0[..., ::97], torch.from_numpy(g2[f"hd{hd}_delta_nomsg_sub"]), f"hd{hd} delta, no message (element-wise)", atol_of_max=5e-6)
        lg = D(s.to(dev) + d)
        assert lg.shape == (2, 17, 16000)
        assert rel(lg[..., ::97], torch.from_numpy(g2[f"hd{hd}_logits_sub"])) <= TOL
        check_elementwise(lg[..., ::97], torch.from_numpy(g2[f"hd{hd}_logits_sub"]), f"hd{hd} logits (element-wise)", atol_of_max=5e-6)
        # a different batch / length against the oracle directly
        s3 = O.synthetic_clips(3, seed=77, T=8000)
        m3 = torch.tensor([1, 2, 65535])
        assert rel(G(s3.to(dev), m3.to(dev)), O2.generator_forward(gsd, s3, m3)) <= TOL
        assert rel(D(s3.to(dev)), O2.detector_forward(dsd, s3)) <= TOL


@pytest.mark.parametrize("hd", [256, 32])
def test_main14b2_backward_vs_oracle(M, hd):
    """every parameter gradient (and the input gradient of the Detector) of the deep-residual variant against the
    oracle's CPU autograd, for a fixed random linear functional of delta and of the logits"""
    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    G, D = M.Generator(hidden_dim=hd), M.Detector()
    gsd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in G.state_dict().items()}
    dsd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in D.state_dict().items()}
    G.to(dev).train(); D.to(dev).train()
    B, T = 2, 8000
    s = O.synthetic_clips(B, seed=21, T=T)
    msg = torch.tensor([7, 7])                      # duplicate rows exercise the embedding scatter-add
    r1, r2 = rnd(B, 1, T, seed=22), rnd(B, 17, T, seed=23)
    # oracle
    d_ref = O2.generator_forward(gsd, s, msg)
    x_in = (s + d_ref.detach()).requires_grad_()
    lg_ref = O2.detector_forward(dsd, x_in)
    ((d_ref * r1).sum() + (lg_ref * r2).sum()).backward()
    # HIP
    d = G(s.to(dev), msg.to(dev))
    x_in_h = (s.to(dev) + d.detach()).requires_grad_()
    lg = D(x_in_h)
    assert rel(d, d_ref) <= TOL and rel(lg, lg_ref) <= TOL
    ((d * r1.to(dev)).sum() + (lg * r2.to(dev)).sum()).backward()
    assert rel(x_in_h.grad, x_in.grad) <= 2e-3, "detector input gradient"
    worst = ("", 0.0)
    for name, mod, ref in (("G", G, gsd), ("D", D, dsd)):
        for k, p in mod.named_parameters():
            assert p.grad is not None, f"{name}.{k} has no gradient"
            e = rel(p.grad, ref[k].grad)
            if e > worst[1]:
                worst = (f"{name}.{k}", e)
            assert e <= 2e-3, f"{name}.{k}: grad rel err {e:.3e}"
    print("worst grad rel err", worst)


def test_main14b2_train_step_vs_oracle(M):
    """config-5 step recipe (clamped s_w, channel-first logits, 5 weighted loss terms): values and a few gradients"""
    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    G, D = M.Generator(hidden_dim=256), M.Detector()
    gsd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in G.state_dict().items()}
    dsd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in D.state_dict().items()}
    G.to(dev).train(); D.to(dev).train()
    s = O.synthetic_clips(2, seed=31)
    msg = torch.tensor([123, 45678])
    tot_r, out_r = O2.step_losses(gsd, dsd, s, msg)
    tot_r.backward()
    tot, out = M.forward_losses(G, D, s.to(dev), msg.to(dev))
    tot.backward()
    for k in ("l1", "mel", "loud", "loc", "bce", "raw_total", "total"):
        assert rel(out[k].reshape(1), out_r[k].reshape(1)) <= TOL, k
    assert rel(out["logits"], out_r["logits"]) <= TOL
    for name, mod, ref in (("G", G, gsd), ("D", D, dsd)):
        for k, p in mod.named_parameters():
            assert rel(p.grad, ref[k].grad) <= 3e-3, f"{name}.{k}"


def test_full_size_properties_b128(M):
    """BASELINE configs[4] size (B = 128 clips x 16 000 samples, hidden 256), through size-independent properties:
    (1) clips are independent units (no BatchNorm in this variant): a clip's delta / logits are bit-identical whether it runs
        alone or inside the batch of 128 (tile / workgroup mapping, split-K grids, LSTM batch tiles leak nothing);
    (2) the whole train step is bit-reproducible: the weight gradients are split-K slabs reduced in a fixed order (no float
        atomics anywhere), so two runs from the same state give identical losses and identical updated parameters;
    (3) permuting the batch permutes delta exactly and leaves every loss term unchanged up to fp32 summation order."""
    import awm_amd
    dev = torch.device("cuda:0")
    B = 128
    s = O.synthetic_clips(B, seed=123).to(dev)
    msg = O.synthetic_messages(B, seed=124).to(dev)

    def fresh():
        torch.manual_seed(42)
        G, D = M.Generator(hidden_dim=256), M.Detector()
        return G.to(dev).train(), D.to(dev).train()
    G, D = fresh()
    pick = [0, 1, 77, 127]
    with torch.no_grad():
        d_all = G(s, msg)
        lg_all = D(s + d_all)
        d_few = G(s[pick], msg[pick])
        lg_few = D(s[pick] + d_few)
    assert torch.equal(d_all[pick], d_few), float((d_all[pick] - d_few).abs().max())
    assert torch.equal(lg_all[pick], lg_few), float((lg_all[pick] - lg_few).abs().max())
    assert torch.isfinite(lg_all).all() and lg_all.shape == (B, 17, 16000)
    del d_all, lg_all, d_few, lg_few
    runs = []
    for _ in range(2):
        G, D = fresh()
        opt = awm_amd.FlatAdam([G, D], lr=1e-3)
        out = M.train_step(G, D, opt, s, msg)
        torch.cuda.synchronize()
        runs.append(({k: float(out[k]) for k in ("l1", "mel", "loud", "loc", "bce", "total")}, opt.flat.clone(), opt.grad.clone()))
        del out, opt
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert torch.equal(runs[0][2], runs[1][2]), "gradients differ between two identical runs"
    assert torch.equal(runs[0][1], runs[1][1]), "updated parameters differ between two identical runs"
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(5)).to(dev)
    G, D = fresh()
    with torch.no_grad():
        _, oa = M.forward_losses(G, D, s, msg)
        _, ob = M.forward_losses(G, D, s[perm], msg[perm])
    assert torch.equal(ob["delta"], oa["delta"][perm])
    for k in ("total", "loc", "bce", "l1", "mel", "loud"):
        a, b = float(oa[k]), float(ob[k])
        assert abs(a - b) <= 1e-5 * max(abs(a), abs(b), 1e-6) + 1e-7, (k, a, b)
