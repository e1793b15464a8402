"""Kernel-level checks of the main14b_2 (BASELINE config 5) generic convolution family against plain fp64 CPU references.

Two kinds of check:
  * exact probes -- integer-valued inputs with sum |products| < 2^24 per output: every product and partial sum is exact in fp32 (and the
    f16 pieces of such inputs have lo = 0), so the kernel must equal the fp64 reference cast to fp32 bit for bit, whatever the summation
    order, tiling or split-K depth.  Any indexing / tiling / split-K / remap error shows, however small its numeric effect.
  * fp64 random tests -- element-wise bars of check_elementwise (rtol 1e-4, 1e-6 of max): the arithmetic (f16 lo pieces, scales, ELU
    epilogue, LSTM cell).
"""
import ctypes
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_gpu_main14b2 import check_elementwise, rel, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXACT = 2.0 ** 24


@pytest.fixture(scope="module")
def M():
    import awm_amd
    awm_amd.lib.load()
    from awm_amd import main14b_2
    return main14b_2


def ints(*shape, seed, lo=-2, hi=2, density=1.0):
    """small integers in [lo, hi], a fraction `density` of them non-zero-by-construction"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(lo, hi + 1, shape, generator=g).float()
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density).float()
    return v


# ------------------------------------------------------------------------------------------ wm_gwgrad
GW_RA, GW_RB = 16, 24


def gw_plan(NB, Ca, Cb, La, K):
    """mirror of gw_plan (csrc/gconv_wgrad.hip) -- only to report / assert which paths the cases take; its split-K depth is checked
    against the library's own workspace size (wm_gwgrad_plan), so a drifted mirror fails loudly instead of mis-reporting"""
    WA = 2 if Ca > 32 else 1
    TA, R, NJ = 32 * WA, 4 // WA, Cb * K
    nta = (Ca + TA - 1) // TA
    nsub_total = (NJ + 31) // 32
    bw = bn = 1
    best_waste, best_tj = 1 << 30, 0
    wjw = R
    while wjw >= 1:
        for ns in (4, 3, 2, 1):
            tjb = wjw * ns
            if tjb > nsub_total and not (wjw == 1 and ns == 1) and (tjb - nsub_total) >= ns:
                continue
            rows = min((tjb * 32 - 1) // K + 2, Cb)
            if rows > 4 * GW_RB and not (wjw == 1 and ns == 1):
                continue
            waste = ((nsub_total + tjb - 1) // tjb) * tjb - nsub_total
            if waste < best_waste or (waste == best_waste and tjb > best_tj):
                best_waste, best_tj, bw, bn = waste, tjb, wjw, ns
        wjw >>= 1
    WJW, nsub = bw, bn
    WT = R // WJW
    TJ = WJW * 32 * nsub
    NBCH = min((TJ - 1) // K + 2, Cb)
    ntj = (NJ + TJ - 1) // TJ
    ra, rbx = min(Ca, TA), NBCH
    plan = None
    for ncb in (4, 3, 2, 1):
        for narrow in (0, 1):
            if plan is not None or (narrow and ncb > 1):
                continue
            width = 32 if narrow else 64 * ncb
            tcmax = (width - (K - 1)) & ~7
            if tcmax < 8 or (not narrow and ncb > 1 and La < 64 * (ncb - 1)) or (not narrow and ncb == 1 and La <= 24):
                continue
            nchunks = -(-La // tcmax)
            TC = min((-(-La // nchunks) + 7) & ~7, tcmax)
            nchunks = -(-La // TC)
            rpu = 2 if TC + K - 1 <= 32 else 1
            if (rpu == 2) != (narrow == 1):
                continue
            a_units, b_units = -(-ra // rpu) * ncb, -(-rbx // rpu) * ncb
            AP, bpw = (width + 2) | 1, width + 2
            BP = bpw + (K - bpw) % 32
            lds = max((TA * AP + (NBCH + 1) * BP) * 4, (WT - 1) * WA * WJW * 4 * 16 * 64 * 4, 4096)
            if a_units <= 4 * GW_RA and b_units <= 4 * GW_RB and lds <= 52 * 1024:
                plan = dict(WA=WA, WJW=WJW, nsub=nsub, WT=WT, ncb=ncb, narrow=bool(narrow), TC=TC, nchunks=nchunks,
                            geo1=ncb == 1 and TC + K - 1 > 32)
    assert plan is not None
    nwork = NB * plan["nchunks"]
    tiles = nta * ntj
    plan["nwork"] = nwork
    plan["gz"] = max(1, min(1 if tiles >= 768 else 768 // tiles, nwork))
    return plan


def lib_gz(M, NB, Ca, Cb, La, K):
    out = (ctypes.c_longlong * 1)()
    M.lib.wm_gwgrad_plan(NB, Ca, Cb, La, K, ctypes.addressof(out), None)
    slab = int(out[0])
    assert slab % (Ca * (Cb * K + 1)) == 0
    return slab // (Ca * (Cb * K + 1))


def positions(NB, La, density, seed):
    """(nb, t) of the non-zero columns of a probe: every position, or a random `density` share of them plus both ends of every clip"""
    if density >= 1.0:
        nb, t = torch.meshgrid(torch.arange(NB), torch.arange(La), indexing="ij")
        return nb.reshape(-1), t.reshape(-1)
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(NB, La, generator=g) < density
    m[:, 0] = True
    m[:, -1] = True
    nb, t = m.nonzero(as_tuple=True)
    return nb, t


def gw_windows(Bx, nb, t, K, P):
    """[n][Cb][K]: Bx[nb][b][t + k - P], zero outside [0, Lb)"""
    Lb = Bx.shape[2]
    cols = []
    for k in range(K):
        u = t + k - P
        ok = ((u >= 0) & (u < Lb)).to(Bx.dtype)
        cols.append(Bx[nb, :, u.clamp(0, Lb - 1)] * ok[:, None])
    return torch.stack(cols, 2)


def gw_remap(G, remap, r1, r2):
    """the column order wm_gwgrad's reduce writes: G [Ca][Cb*K] in the GEMM's own order (column b*K + k) -> the weight's order"""
    Ca = G.shape[0]
    if remap == 1:      # column k*r1 + b -> b*r2 + k   (tap planes -> dW[a][b][k])
        return G.reshape(Ca, r2, r1).permute(0, 2, 1).reshape(Ca, -1)
    if remap == 2:      # column (co*r1 + ph)*2 + q -> co*2*r1 + q*r1 + ph   (stride phases -> ConvTranspose taps)
        return G.reshape(Ca, -1, r1, 2).permute(0, 1, 3, 2).reshape(Ca, -1)
    return G


def gw_probe(NB, Ca, Cb, La, Lb, K, P, bcs=0, seed=0, budget=2.5e8):
    """integer probe of wm_gwgrad on the GPU: A non-zero at `positions` (all channels), Bx dense small integers (inside a wider clip
    row when bcs > Cb*Lb); returns (A, Bx view, fp64 reference G [Ca][Cb*K] in GEMM order, fp64 dbias)"""
    dens = min(1.0, budget / (NB * La * Ca * Cb * K))
    nb, t = positions(NB, La, dens, seed)
    g = torch.Generator(device=DEV).manual_seed(seed)
    A = torch.zeros(NB, Ca, La, device=DEV)
    av = torch.randint(-2, 3, (nb.numel(), Ca), generator=g, device=DEV).float()
    A[nb.to(DEV), :, t.to(DEV)] = av
    width = bcs if bcs else Cb * Lb
    W = torch.randint(-2, 3, (NB, width), generator=g, device=DEV).float()
    off = (width - Cb * Lb) // 2
    Bx = W[:, off:off + Cb * Lb].view(NB, Cb, Lb)
    win = gw_windows(Bx, nb.to(DEV), t.to(DEV), K, P).reshape(nb.numel(), Cb * K).double().cpu()
    av = av.double().cpu()
    G = av.t() @ win
    bound = float((av.abs().t() @ win.abs()).max())
    assert bound < EXACT and float(av.abs().sum(0).max()) < EXACT, f"probe not exact in fp32: sum |products| = {bound:g}"
    return A, Bx, G, av.sum(0)


# (NB, Ca, Cb, La, Lb, K, P, bcs, remap, r1, r2, dbias): remap 1 = tap planes (K = 1, Cb = K' * C), remap 2 = ConvTranspose phases
GW_CASES = [
    (2, 17, 5, 63, 63, 3, 1, 0, 0, 0, 0, True),
    (3, 33, 7, 130, 130, 7, 3, 0, 0, 0, 0, False),
    (2, 48, 16, 200, 200, 3, 1, 0, 0, 0, 0, True),
    (1, 8, 8, 1, 1, 3, 1, 0, 0, 0, 0, True),
    (3, 16, 4, 1, 1, 7, 3, 0, 0, 0, 0, False),
    (4, 32, 32, 8, 8, 2, 0, 0, 0, 0, 0, True),
    (5, 24, 10, 24, 24, 1, 0, 0, 0, 0, 0, True),
    (3, 64, 64, 25, 25, 3, 1, 0, 0, 0, 0, False),
    (2, 16, 16, 64, 64, 7, 3, 0, 0, 0, 0, True),
    (2, 20, 9, 77, 80, 2, 1, 0, 0, 0, 0, True),
    (2, 40, 11, 190, 187, 3, 1, 0, 0, 0, 0, False),
    (2, 64, 32, 16000, 16000, 3, 1, 0, 0, 0, 0, True),
    (2, 8, 8, 16000, 16000, 3, 1, 0, 0, 0, 0, True),
    (2, 1024, 2048, 64, 64, 1, 0, 0, 0, 0, 0, True),
    (33, 1024, 256, 50, 50, 1, 0, 0, 0, 0, 0, True),
    (3, 64, 96, 250, 250, 1, 0, 0, 1, 32, 3, True),
    (2, 128, 192, 100, 100, 1, 0, 3 * 64 * 100 + 0, 1, 64, 3, True),
    (2, 128, 64, 100, 100, 1, 0, 3 * 64 * 100, 0, 0, 0, True),
    (2, 33, 17, 130, 130, 1, 0, 17 * 130 + 77, 0, 0, 0, False),
    (2, 32, 80, 130, 131, 2, 0, 0, 2, 5, 0, False),
    (2, 64, 256, 50, 51, 2, 0, 0, 2, 8, 0, False),
    (3, 16, 16, 1003, 1004, 2, 0, 0, 2, 2, 0, False),
    (2, 20, 9, 600, 600, 3, 1, 0, 0, 0, 0, True),
]


def _gw_id(c):
    return "NB{}_Ca{}_Cb{}_La{}_Lb{}_K{}_P{}_bcs{}_remap{}".format(*c[:9])


def test_gwgrad_cases_cover_the_plan(M):
    """the synthetic shapes below hit every branch of gw_plan the issue lists (the mirror's split-K depth = the library's)"""
    seen = dict(WA=set(), ncb=set(), narrow=set(), geo1=set(), nsub=set(), WT=set(), K=set(), P=set(), remap=set(), dbias=set())
    gz_kinds, la, ca_kinds = set(), set(), set()
    for (NB, Ca, Cb, La, Lb, K, P, bcs, remap, r1, r2, db) in GW_CASES:
        p = gw_plan(NB, Ca, Cb, La, K)
        assert p["gz"] == lib_gz(M, NB, Ca, Cb, La, K), (NB, Ca, Cb, La, K, p)
        for k in ("WA", "ncb", "narrow", "geo1", "nsub", "WT"):
            seen[k].add(p[k])
        seen["K"].add(K); seen["P"].add(P); seen["remap"].add(remap); seen["dbias"].add(db)
        la.add(La)
        ca_kinds.add("le32" if Ca <= 32 else ("32_64" if Ca < 64 else "big"))
        if Ca % 32:
            ca_kinds.add(f"odd{Ca}")
        if p["gz"] == 1 and p["nwork"] > 1:
            gz_kinds.add("one")
        if p["gz"] == p["nwork"]:
            gz_kinds.add("all")
        if 1 < p["gz"] < p["nwork"] and p["nwork"] % p["gz"]:
            gz_kinds.add("ragged")
    print(seen, gz_kinds)
    assert seen["WA"] == {1, 2} and seen["ncb"] == {1, 2, 3, 4} and seen["narrow"] == {False, True} and seen["geo1"] == {False, True}
    assert {1, 2, 4} <= seen["WT"] and len(seen["nsub"]) >= 3
    assert {1, 2, 3, 7} <= seen["K"] and {0, 1, 3} <= seen["P"] and seen["remap"] == {0, 1, 2} and seen["dbias"] == {False, True}
    assert {1, 8, 24, 25, 63, 64, 130, 200, 16000} <= la
    assert {"le32", "32_64", "big", "odd17", "odd33"} <= ca_kinds and 1024 in {c[1] for c in GW_CASES}
    assert any(c[2] * c[5] % 32 for c in GW_CASES) and any(c[7] > c[2] * c[4] for c in GW_CASES)
    assert gz_kinds == {"one", "all", "ragged"}, gz_kinds


@pytest.mark.parametrize("case", GW_CASES, ids=_gw_id)
def test_gwgrad_exact(M, case):
    NB, Ca, Cb, La, Lb, K, P, bcs, remap, r1, r2, db = case
    A, Bx, G, dbias = gw_probe(NB, Ca, Cb, La, Lb, K, P, bcs, seed=GW_CASES.index(case))
    out, dbo = M._gwgrad_raw(A, Bx, Cb, Lb, bcs, (Ca, Cb * K), K, P, db, remap, r1, r2)
    want = gw_remap(G, remap, r1, r2).float()
    got = out.reshape(Ca, -1).cpu()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} weight-gradient entries differ; max |diff| " \
                                   f"{float((got - want).abs().max()):g}"
    if db:
        assert torch.equal(dbo.cpu(), dbias.float())


@pytest.mark.parametrize("case", [GW_CASES[0], GW_CASES[11], GW_CASES[15], GW_CASES[19]], ids=_gw_id)
def test_gwgrad_accumulate_exact(M, case):
    """accumulate = 1 adds onto a pre-filled G / dbias (what the side-stream path of the flat gradient bucket relies on)"""
    NB, Ca, Cb, La, Lb, K, P, bcs, remap, r1, r2, _ = case
    A, Bx, G, dbias = gw_probe(NB, Ca, Cb, La, Lb, K, P, bcs, seed=7)
    G0, d0 = ints(Ca, Cb * K, seed=8, lo=-1000, hi=1000), ints(Ca, seed=9, lo=-1000, hi=1000)
    Gd, dd = G0.to(DEV), d0.to(DEV)
    slab = M._gwgrad_workspace(NB, Ca, Cb, La, K, A.device)
    M.lib.wm_gwgrad(A.data_ptr(), Bx.data_ptr(), Gd.data_ptr(), dd.data_ptr(), slab.data_ptr(), NB, Ca, Cb, La, Lb, K, P, bcs, remap, r1,
                    r2, 1, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(Gd.cpu(), (G0.double() + gw_remap(G, remap, r1, r2)).float())
    assert torch.equal(dd.cpu(), (d0.double() + dbias).float())


@pytest.mark.parametrize("case,offset", [(GW_CASES[2], 0.0), (GW_CASES[11], 0.0), (GW_CASES[11], 0.5), (GW_CASES[14], 0.0),
                                         (GW_CASES[16], 0.0), (GW_CASES[20], 0.5)], ids=lambda v: str(v))
def test_gwgrad_fp64_random(M, case, offset):
    """random data; offset > 0 makes every operand positive, so every chunk adds to every output and a lost one cannot cancel out"""
    NB, Ca, Cb, La, Lb, K, P, bcs, remap, r1, r2, db = case
    A = rnd(NB, Ca, La, seed=41)
    W = rnd(NB, bcs if bcs else Cb * Lb, seed=42)
    if offset:
        A, W = A.abs() + offset, W.abs() + offset
    off = ((bcs if bcs else Cb * Lb) - Cb * Lb) // 2
    Bx = W[:, off:off + Cb * Lb].reshape(NB, Cb, Lb)
    nb, t = positions(NB, La, 1.0, 0)
    G = A.double()[nb, :, t].t() @ gw_windows(Bx.double(), nb, t, K, P).reshape(nb.numel(), -1)
    Wd = W.to(DEV)
    out, dbo = M._gwgrad_raw(A.to(DEV), Wd[:, off:off + Cb * Lb].view(NB, Cb, Lb), Cb, Lb, bcs, (Ca, Cb * K), K, P, True, remap, r1, r2)
    check_elementwise(out.reshape(Ca, -1), gw_remap(G, remap, r1, r2), "dW")
    check_elementwise(dbo, A.double().sum((0, 2)), "db")


def test_gwgrad_production_shapes_exact(M, monkeypatch):
    """one config-5 train step (B = 128, hidden 256, T = 16 000) with wm_gwgrad / wm_gather_taps recorded; every distinct argument
    tuple is then replayed as an exact probe at that very shape (clips, channels, lengths, taps, padding, clip stride, remap)"""
    import awm_amd
    from oracle import wm_oracle as O
    gw, gt = set(), set()
    o_gw, o_gt = M.lib.wm_gwgrad, M.lib.wm_gather_taps

    def spy_gw(*a):
        gw.add(tuple(int(v) for v in a[5:17]) + (a[3] is not None,))
        return o_gw(*a)

    def spy_gt(*a):
        gt.add(tuple(int(v) for v in a[2:10]))
        return o_gt(*a)
    monkeypatch.setattr(M.lib, "wm_gwgrad", spy_gw)
    monkeypatch.setattr(M.lib, "wm_gather_taps", spy_gt)
    B = 128
    torch.manual_seed(42)
    G, D = M.Generator(hidden_dim=256).to(DEV).train(), M.Detector().to(DEV).train()
    opt = awm_amd.FlatAdam([G, D], lr=1e-3)
    out = M.train_step(G, D, opt, O.synthetic_clips(B, seed=123).to(DEV), O.synthetic_messages(B, seed=124).to(DEV))
    torch.cuda.synchronize()
    del out, opt, G, D
    monkeypatch.undo()
    torch.cuda.empty_cache()
    assert len(gw) >= 20 and len(gt) >= 8, (len(gw), len(gt))
    print(f"{len(gw)} distinct wm_gwgrad shapes, {len(gt)} distinct wm_gather_taps shapes")
    for i, (NB, Ca, Cb, La, Lb, K, P, bcs, remap, r1, r2, acc, db) in enumerate(sorted(gw)):
        assert acc == 0
        A, Bx, Gr, dbias = gw_probe(NB, Ca, Cb, La, Lb, K, P, bcs, seed=100 + i)
        got, dbo = M._gwgrad_raw(A, Bx, Cb, Lb, bcs, (Ca, Cb * K), K, P, db, remap, r1, r2)
        want = gw_remap(Gr, remap, r1, r2).float()
        got = got.reshape(Ca, -1).cpu()
        assert torch.equal(got, want), (NB, Ca, Cb, La, Lb, K, P, bcs, remap, r1, r2, int((got != want).sum()))
        if db:
            assert torch.equal(dbo.cpu(), dbias.float()), (NB, Ca, Cb, La, K)
        del A, Bx
    for (NB, C, Lin, K, S, P, Lout, order) in sorted(gt):
        x = torch.randn(NB, C, Lin, generator=torch.Generator().manual_seed(NB + C + Lin))
        y = M._gather_taps(x.to(DEV), K, S, P, Lout, order).cpu()
        assert torch.equal(y, gather_ref(x, K, S, P, Lout, order)), (NB, C, Lin, K, S, P, Lout, order)


# ------------------------------------------------------------------------------------------ data movement and reductions
def gather_ref(x, K, S, P, Lout, order):
    NB, C, Lin = x.shape
    xp = F.pad(x, (P, max(0, (Lout - 1) * S + K - P - Lin)))
    planes = torch.stack([xp[:, :, k:k + (Lout - 1) * S + 1:S] for k in range(K)], 1)    # [NB][K][C][Lout]
    if order:
        planes = planes.transpose(1, 2)
    return planes.reshape(NB, C * K, Lout)


@pytest.mark.parametrize("NB,C,Lin,K,S,P,Lout,order", [(2, 3, 1000, 3, 2, 1, 500, 0), (3, 5, 999, 3, 8, 1, 130, 0), (2, 4, 700, 16, 8, 0, 90, 1),
                                                       (1, 7, 301, 8, 8, 4, 40, 1), (2, 2, 50, 5, 5, 2, 300, 1), (4, 3, 1, 7, 1, 3, 257, 0),
                                                       (2, 6, 2000, 4, 4, 2, 513, 1), (3, 2, 333, 2, 3, 5, 111, 0)])
def test_gather_taps_exact(M, NB, C, Lin, K, S, P, Lout, order):
    """S up to 8, K up to 16, P > 0, Lout past the clip (zero fill), lengths off the 256-position tile"""
    x = torch.randn(NB, C, Lin, generator=torch.Generator().manual_seed(K * S + Lin))
    y = M._gather_taps(x.to(DEV), K, S, P, Lout, order).cpu()
    assert torch.equal(y, gather_ref(x, K, S, P, Lout, order))


@pytest.mark.parametrize("A,C,L", [(1, 1, 1), (3, 17, 50), (128, 256, 50), (5, 3, 257)])
def test_permute_acl_exact(M, A, C, L):
    x = torch.randn(A, C, L, generator=torch.Generator().manual_seed(A + C + L))
    xd, y = x.to(DEV), torch.empty(L, C, A, device=DEV)          # device tensors held until the launch has run
    M.lib.wm_permute_acl(xd.data_ptr(), y.data_ptr(), A, C, L, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(y.cpu(), x.permute(2, 1, 0))


@pytest.mark.parametrize("V,Dm,Bn", [(10, 300, 40), (65536, 256, 128), (3, 1, 7)])
def test_rows_scatter_add_exact(M, V, Dm, Bn):
    """duplicate ids add in order onto a pre-filled table (integers: exact)"""
    g = torch.Generator().manual_seed(V + Dm)
    idx = torch.randint(0, min(V, 9), (Bn,), generator=g)
    idx[: Bn // 3] = idx[0]
    dv, t0 = ints(Bn, Dm, seed=V, lo=-50, hi=50), ints(V, Dm, seed=Dm, lo=-50, hi=50)
    dt, idxd, dvd = t0.to(DEV), idx.to(DEV), dv.to(DEV)
    M.lib.wm_rows_scatter_add(dt.data_ptr(), idxd.data_ptr(), dvd.data_ptr(), Bn, Dm, V, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(dt.cpu(), t0.double().index_add(0, idx, dv.double()).float())


@pytest.mark.parametrize("NB,C,L", [(1, 1, 1), (3, 17, 257), (130, 8, 1003), (256, 32, 300)])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_channel_sum_exact(M, NB, C, L, accumulate):
    x = ints(NB, C, L, seed=NB * C, lo=-3, hi=3)
    assert float(x.abs().sum((0, 2)).max()) < EXACT
    out0 = ints(C, seed=5, lo=-99, hi=99)
    out, xd, part = out0.to(DEV), x.to(DEV), torch.empty(64 * C, device=DEV)
    M.lib.wm_channel_sum(xd.data_ptr(), out.data_ptr(), part.data_ptr(), NB, C, L, accumulate, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(out.cpu(), (x.double().sum((0, 2)) + (out0.double() if accumulate else 0)).float())


@pytest.mark.parametrize("rows,L", [(1, 1), (7, 255), (300, 257), (2, 16001)])
def test_rowsum_any_exact(M, rows, L):
    x = ints(rows, L, seed=rows + L, lo=-5, hi=5)
    xd, out = x.to(DEV), torch.empty(rows, device=DEV)
    M.lib.wm_rowsum_any(xd.data_ptr(), out.data_ptr(), rows, L, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(out.cpu(), x.double().sum(1).float())


# ------------------------------------------------------------------------------------------ LSTM
@pytest.mark.parametrize("H", [32, 64, 256])
@pytest.mark.parametrize("B", [1, 16, 17, 32, 33, 128])
def test_lstm_layer_vs_nn_lstm(M, H, B):
    """LSTMLayerFn (time-major [T][H][B], batch tiles of 32 forward / 16 backward) against nn.LSTM(H, H) in double: h, dx and the four
    parameter gradients (b_ih and b_hh receive the same db).  B = 128, H = 256, T = 50 is the production shape."""
    for T in (1, 2, 50):
        torch.manual_seed(H * 1000 + B * 10 + T)
        ref = nn.LSTM(H, H).double()
        x, dout = rnd(T, B, H, seed=T + 1), rnd(T, B, H, seed=T + 2)
        xr = x.double().requires_grad_()
        hr, _ = ref(xr)
        hr.backward(dout.double())
        names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
        ps = [getattr(ref, n).detach().float().to(DEV).requires_grad_() for n in names]
        seq = x.permute(0, 2, 1).contiguous().to(DEV).requires_grad_()
        h = M.LSTMLayerFn.apply(seq, *ps)
        h.backward(dout.permute(0, 2, 1).contiguous().to(DEV))
        tag = f"H{H} B{B} T{T}"
        check_elementwise(h.permute(0, 2, 1), hr, f"{tag} h")
        check_elementwise(seq.grad.permute(0, 2, 1), xr.grad, f"{tag} dx")
        for n, p in zip(names, ps):
            check_elementwise(p.grad, getattr(ref, n).grad, f"{tag} d{n}")


# ------------------------------------------------------------------------------------------ autograd Functions
def _uni(*shape, fan_in, seed):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1) / math.sqrt(fan_in)


RB_SHAPES = [(32, 64, 2, 1002), (64, 128, 4, 1001), (128, 256, 5, 402), (256, 512, 8, 403),
             (256, 256, 1, 203), (128, 128, 1, 301), (64, 64, 1, 1000), (64, 64, 1, 998), (32, 32, 1, 999), (16, 16, 1, 1001), (8, 8, 1, 777)]


@pytest.mark.parametrize("cin,cout,stride,L", RB_SHAPES)
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("h", [True, False])
def test_residual_block_fn_vs_fp64(M, cin, cout, stride, L, fused, h):
    """every (Cin, Cout, stride) block the Generator / Detector build, at ragged lengths; fused strided data gradient on / off,
    f16 split on / off: output, dx and all six parameter gradients"""
    if not fused and not (stride >= 3 and cin != cout):
        pytest.skip("the fused strided data gradient only exists for down-sampling blocks with stride >= 3")
    skip = stride != 1 or cin != cout
    s = cin * 7 + cout + stride
    w1, b1 = _uni(cout, cin, 3, fan_in=cin * 3, seed=s), _uni(cout, fan_in=cin * 3, seed=s + 1)
    w2, b2 = _uni(cout, cout, 3, fan_in=cout * 3, seed=s + 2), _uni(cout, fan_in=cout * 3, seed=s + 3)
    ws, bs = (_uni(cout, cin, 1, fan_in=cin, seed=s + 4), _uni(cout, fan_in=cin, seed=s + 5)) if skip else (None, None)
    x = rnd(2, cin, L, seed=s + 6)
    params = [w1, b1, w2, b2] + ([ws, bs] if skip else [])
    xr, pr = x.double().requires_grad_(), [p.double().requires_grad_() for p in params]
    out1 = F.elu(F.conv1d(xr, pr[0], pr[1], stride=stride, padding=1))
    res = F.conv1d(xr, pr[4], pr[5], stride=stride) if skip else xr
    yr = F.elu(F.conv1d(out1, pr[2], pr[3], padding=1) + res)
    gy = rnd(*yr.shape, seed=s + 7)
    yr.backward(gy.double())
    xd, pd = x.to(DEV).requires_grad_(), [p.to(DEV).requires_grad_() for p in params]
    with M.ops.switches(gconv_f16x3=h, fused_strided_dgrad=fused):
        y = M.ResidualBlockFn.apply(xd, pd[0], pd[1], pd[2], pd[3], pd[4] if skip else None, pd[5] if skip else None, stride)
        y.backward(gy.to(DEV))
    check_elementwise(y, yr, "y")
    check_elementwise(xd.grad, xr.grad, "dx")
    for n, a, r in zip(("dw1", "db1", "dw2", "db2", "dws", "dbs"), pd, pr):
        check_elementwise(a.grad, r.grad, n)


CT_SHAPES = [(512, 256, 8, 50), (256, 128, 5, 77), (128, 64, 4, 301), (64, 32, 2, 999),
             (128, 64, 8, 50), (64, 32, 5, 400), (32, 16, 4, 501), (16, 8, 2, 1003)]


@pytest.mark.parametrize("cin,cout,st,L", CT_SHAPES)
def test_convT_fn_vs_fp64(M, cin, cout, st, L):
    """all eight ConvTranspose1d(k = 2 st, stride st, padding st / 2) layers of the Detector and the Generator: y, dx, dW, db"""
    w, b = _uni(cin, cout, 2 * st, fan_in=cout * 2 * st, seed=cin + st), _uni(cout, fan_in=cout * 2 * st, seed=cin + st + 1)
    x = rnd(2, cin, L, seed=cin + 2)
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    yr = F.conv_transpose1d(xr, wr, br, stride=st, padding=st // 2)
    g = rnd(*yr.shape, seed=cin + 3)
    yr.backward(g.double())
    xd, wd, bd = (t.to(DEV).requires_grad_() for t in (x, w, b))
    y = M.ConvTFn.apply(xd, wd, bd, st)
    y.backward(g.to(DEV))
    for n, a, r in (("y", y, yr), ("dx", xd.grad, xr.grad), ("dw", wd.grad, wr.grad), ("db", bd.grad, br.grad)):
        check_elementwise(a, r, n)


# (Cin, Cout, K, stride, padding, act, with res, with vec)
CONV_CASES = [(32, 48, 3, 1, 1, 1, False, False), (32, 48, 3, 1, 1, 0, True, False), (48, 32, 3, 1, 1, 1, True, False),
              (1, 32, 7, 1, 3, 0, False, False), (512, 256, 1, 1, 0, 0, False, True), (256, 128, 7, 1, 3, 0, False, False),
              (32, 17, 7, 1, 3, 0, False, False), (8, 1, 7, 1, 3, 0, False, False), (32, 64, 1, 2, 0, 1, False, True)]


@pytest.mark.parametrize("cin,cout,k,stride,pad,act,has_res,has_vec", CONV_CASES)
@pytest.mark.parametrize("grad_rows", [0, 1, 3])
def test_conv_fn_vs_fp64(M, cin, cout, k, stride, pad, act, has_res, has_vec, grad_rows):
    """ConvFn: ELU on / off, residual input, per-clip vector (the K = 1 proj + embedding path), input gradient for the first
    grad_rows clips only (the rest exactly zero)"""
    NB, L = 3, (50 if has_vec and stride == 1 else 333)
    s = cin + cout + k
    w, b = _uni(cout, cin, k, fan_in=cin * k, seed=s), _uni(cout, fan_in=cin * k, seed=s + 1)
    x = rnd(NB, cin, L, seed=s + 2)
    Lout = (L + 2 * pad - k) // stride + 1
    res = rnd(NB, cout, Lout, seed=s + 3) if has_res else None
    vec = rnd(NB, cout, seed=s + 4) if has_vec else None
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    resr = res.double().requires_grad_() if has_res else None
    vecr = vec.double().requires_grad_() if has_vec else None
    z = F.conv1d(xr, wr, br, stride=stride, padding=pad)
    if has_vec:
        z = z + vecr[:, :, None]
    if has_res:
        z = z + resr
    yr = F.elu(z) if act else z
    g = rnd(*yr.shape, seed=s + 5)
    yr.backward(g.double())
    xd, wd, bd = (t.to(DEV).requires_grad_() for t in (x, w, b))
    resd = res.to(DEV).requires_grad_() if has_res else None
    vecd = vec.to(DEV).requires_grad_() if has_vec else None
    y = M.ConvFn.apply(xd, wd, bd, stride, pad, act, resd, vecd, grad_rows)
    y.backward(g.to(DEV))
    check_elementwise(y, yr, "y")
    dx_want = xr.grad.clone()
    if stride == 1:                      # only clips [0, grad_rows) get an input gradient; the rest is exactly zero
        dx_want[grad_rows:] = 0
    check_elementwise(xd.grad, dx_want, "dx")
    if stride == 1:
        assert not xd.grad[grad_rows:].any()
    check_elementwise(wd.grad, wr.grad, "dw")
    check_elementwise(bd.grad, br.grad, "db")
    if has_res:
        check_elementwise(resd.grad, resr.grad, "dres")
    if has_vec:
        check_elementwise(vecd.grad, vecr.grad, "dvec")


@pytest.mark.parametrize("cin,cout,stride,L", [(64, 128, 4, 1001), (128, 256, 5, 402), (256, 512, 8, 403)])
def test_strided_block_dgrad_small_source(M, cin, cout, stride, L):
    """one launch, two gradient sources sharing one f16 scale (set by the larger): gz1 ~ 1e-4 gz2.  The positions only conv1's outer
    taps reach (t S - 1, t S + 1) carry gz1 alone and are checked against their own maximum, so a lost small source cannot hide"""
    w1, ws = _uni(cout, cin, 3, fan_in=cin * 3, seed=cin), _uni(cout, cin, 1, fan_in=cin, seed=cin + 1)
    Lo = (L + 2 - 3) // stride + 1
    gz1, gz2 = rnd(2, cout, Lo, seed=cin + 2, scale=1e-4), rnd(2, cout, Lo, seed=cin + 3)
    ref = (torch.nn.grad.conv1d_input((2, cin, L), w1.double(), gz1.double(), stride=stride, padding=1)
           + torch.nn.grad.conv1d_input((2, cin, L), ws.double(), gz2.double(), stride=stride))
    dx = M._strided_block_dgrad(gz1.to(DEV), w1.to(DEV), gz2.to(DEV), ws.to(DEV), stride, L).cpu()
    check_elementwise(dx, ref, "dx")
    pos = torch.arange(L)
    only1 = (pos % stride == 1) | (pos % stride == stride - 1)
    check_elementwise(dx[..., only1], ref[..., only1], "dx at the positions only gz1 reaches")
    assert not dx[..., ~(only1 | (pos % stride == 0))].any()


def test_rows_gather_fn_backward_duplicates(M):
    """embedding backward: duplicate message ids sum their rows (integers: exact)"""
    table = rnd(20, 256, seed=1).to(DEV).requires_grad_()
    idx = torch.tensor([7, 3, 7, 7, 0, 19, 3, 7])
    g = ints(8, 256, seed=2, lo=-9, hi=9)
    y = M.RowsGatherFn.apply(table, idx.to(DEV))
    assert torch.equal(y.detach().cpu(), table.detach().cpu()[idx])
    y.backward(g.to(DEV))
    assert torch.equal(table.grad.cpu(), torch.zeros(20, 256, dtype=torch.float64).index_add(0, idx, g.double()).float())


# ------------------------------------------------------------------------------------------ activation scale of the f16 split
def _xscaled(shape, xs, seed):
    x = rnd(*shape, seed=seed)
    if xs == "spikes":                   # a few values far outside the f16 range of an unscaled split (+-6e4)
        x[0, 3, 5], x[-1, 1, shape[2] // 2], x[-1, 0, shape[2] - 1] = 1e5, -2e5, 7e4
        return x
    return x * xs


XSCALES = [1e-4, 1e-3, 1e-2, 1.0, 1e3, "spikes"]


def _f16_vs_fp32(run, ref, what):
    """error relative to the result's max: below 1e-6 and within 3x of the native fp32 build + 2e-7 (test_gconv_f16_split_is_fp32_grade's
    bar).  Where the fp32 build itself is above 1e-6 -- the 256-channel k7 layer contracts 1792 products per output, and its fp32
    round-off alone is 1.3-1.7e-6 of max -- the absolute cap is the fp32 build's own error: no arithmetic can be asked to beat fp32 here."""
    outs = [run(h).double().cpu() for h in (False, True)]          # native fp32 MFMA build, f16 split
    e_n = float((outs[0] - ref).abs().max() / ref.abs().max())
    e_h = float((outs[1] - ref).abs().max() / ref.abs().max())
    print(f"{what}: fp32 mfma {e_n:.2e}  f16 split {e_h:.2e}")
    assert e_h < max(1e-6, e_n) and e_h < 3 * e_n + 2e-7, (what, e_n, e_h)


@pytest.mark.parametrize("cin,cout,k,stride,pad,L", [(128, 128, 3, 1, 1, 1001), (32, 64, 3, 2, 1, 1000), (256, 512, 3, 8, 1, 403),
                                                     (512, 256, 1, 1, 0, 50), (256, 128, 7, 1, 3, 50)])
@pytest.mark.parametrize("xs", XSCALES, ids=str)
def test_gconv_h_activation_scale(M, cin, cout, k, stride, pad, L, xs):
    """wm_gconv_h forward (ELU epilogue) for activations of magnitude 1e-4 ... 1e3 and with a few values beyond the f16 range: the same
    bar as test_gconv_f16_split_is_fp32_grade (below 1e-6 of max, within 3x of the fp32 build + 2e-7).  The bias follows the scale of x,
    so the output does too (a unit bias would hide the error of a small x)."""
    x = _xscaled((2, cin, L), xs, seed=51)
    bs = 1.0 if xs == "spikes" else xs
    w, b = rnd(cout, cin, k, seed=52, scale=0.1), rnd(cout, seed=53) * bs
    ref = F.elu(F.conv1d(x.double(), w.double(), b.double(), stride=stride, padding=pad))

    def run(h):
        with torch.no_grad(), M.ops.switches(gconv_f16x3=h):
            return M._gconv(x.to(DEV), w.to(DEV), b.to(DEV), stride, pad, act=1)
    _f16_vs_fp32(run, ref, f"{cin}>{cout} k{k} s{stride} x {xs}")


@pytest.mark.parametrize("cin,cout,st,L", [(128, 64, 8, 50), (32, 16, 4, 501), (16, 8, 2, 1003), (512, 256, 8, 50)])
@pytest.mark.parametrize("xs", XSCALES, ids=str)
def test_gconvT_activation_scale(M, cin, cout, st, L, xs):
    x = _xscaled((2, cin, L), xs, seed=61)
    bs = 1.0 if xs == "spikes" else xs
    w, b = rnd(cin, cout, 2 * st, seed=62, scale=0.1), rnd(cout, seed=63) * bs
    ref = F.conv_transpose1d(x.double(), w.double(), b.double(), stride=st, padding=st // 2)

    def run(h):
        with M.ops.switches(gconv_f16x3=h):
            return M._gconvT(x.to(DEV), w.to(DEV), b.to(DEV), st)
    _f16_vs_fp32(run, ref, f"convT {cin}>{cout} st{st} x {xs}")


@pytest.mark.parametrize("xs", XSCALES, ids=str)
def test_lstm_input_projection_activation_scale(M, xs):
    """the input projection of a 256-unit LSTM layer over 50 steps x 128 clips, as LSTMLayerFn launches it"""
    T, H, B = 50, 256, 128
    seq = _xscaled((T, H, B), xs, seed=71)
    w, b = rnd(4 * H, H, seed=72, scale=0.06), rnd(4 * H, seed=73) * (1.0 if xs == "spikes" else xs)
    ref = torch.einsum("gh,thb->tgb", w.double(), seq.double()) + b.double()[None, :, None]

    def run(h):
        with M.ops.switches(gconv_f16x3=h):
            return M._lstm_proj(seq.to(DEV), w.to(DEV), b.to(DEV))
    _f16_vs_fp32(run, ref, f"lstm projection x {xs}")


def test_activation_scale_is_per_clip(M):
    """the activation scale is one power of two per clip: a clip's result is bit-identical alone and next to a clip 1e4 times larger"""
    x = rnd(3, 128, 700, seed=81)
    x[1] *= 1e4
    x[2] *= 1e-3
    w, b = rnd(256, 128, 3, seed=82, scale=0.1), rnd(256, seed=83)
    with torch.no_grad():
        y_all = M._gconv(x.to(DEV), w.to(DEV), b.to(DEV), 1, 1, act=1)
        for i in (0, 2):
            assert torch.equal(y_all[i:i + 1], M._gconv(x[i:i + 1].to(DEV), w.to(DEV), b.to(DEV), 1, 1, act=1)), i


# ------------------------------------------------------------------------------------------ weight image scaled from max |w|
def _pack_h(M, w, Cin, K, Mtot, scaled, fill):
    """wm_gconv_pack_h's image of w [Cin * K][Mtot] -> (the 2 * Cin * K * Mtot f16 words, the two trailing floats).  scaled: with a real
    scratch (ws from max |w| by wm_gscale_absmax, a call across translation units), else scratch = NULL (the fixed ws = 2^8).  The
    buffer starts as `fill`, so a word a route leaves unwritten differs between two routes given different fills."""
    n = Cin * K * Mtot
    wd, scratch = w.contiguous().to(DEV), torch.zeros(1024, device=DEV)
    wph = torch.full((2 * n + 4,), fill, dtype=torch.int16, device=DEV)
    M.lib.wm_gconv_pack_h(wd.data_ptr(), wph.data_ptr(), scratch.data_ptr() if scaled else None, Cin, K, Mtot,
                          torch.cuda.current_stream().cuda_stream)
    return wph[:2 * n].cpu(), wph[2 * n:].view(torch.float32).cpu()


@pytest.mark.parametrize("Cin,K,Mtot", [(16, 3, 5), (32, 1, 4), (16, 7, 17)])
@pytest.mark.parametrize("e", [-3, 0, 5])
def test_gconv_pack_h_scaled_route(M, Cin, K, Mtot, e):
    """the scratch != NULL branch of wm_gconv_pack_h, which no caller in the package takes (main14b_2 passes NULL): max |w| = 0.75 * 2^e
    lies 0.415 binades under 2^e, so ws = exp2(floor(10 - log2(max))) = 2^(10 - e) whatever the last bit of log2f.  The image must be
    bit for bit the fixed-scale route's (the one test_gconv_f16_split_is_fp32_grade holds to fp64) for w * (ws / 2^8): that rescale is
    a power of two, so both routes split the same v = w * ws."""
    g = torch.Generator().manual_seed(1000 * Cin + 10 * K + Mtot + (e + 3))
    w = (torch.rand(Cin * K, Mtot, generator=g) * 2 - 1) * (0.7 * 2.0 ** e)
    w[(Cin * K) // 2, Mtot // 2] = 0.75 * 2.0 ** e
    ws = 2.0 ** (10 - e)
    img, tail = _pack_h(M, w, Cin, K, Mtot, True, 0x5555)
    assert tail.tolist() == [ws, 1.0 / ws], (tail.tolist(), ws)
    ref, ref_tail = _pack_h(M, w * (ws / 256.0), Cin, K, Mtot, False, 0x2AAA)
    assert ref_tail.tolist() == [256.0, 1.0 / 256.0]
    assert torch.equal(img, ref), f"{int((img != ref).sum())} of {img.numel()} f16 words differ"


def test_gconv_pack_h_scaled_route_all_zero(M):
    """max |w| = 0: the scale is 1 and the image all zero"""
    Cin, K, Mtot = 16, 3, 5
    img, tail = _pack_h(M, torch.zeros(Cin * K, Mtot), Cin, K, Mtot, True, 0x5555)
    assert tail.tolist() == [1.0, 1.0]
    assert not img.any()


# ------------------------------------------------------------------------------------------ gradient scale under in-place accumulation
def test_gradient_scale_after_inplace_accumulation(M, monkeypatch):
    """y0 = ConvFn(x, act 0) feeds two consumers: a ConvFn whose dx comes from wm_gconv_h (it notes max |dx| for y0's gradient) and a
    branch whose gradient is ~100x larger.  The ConvFn branch is created last, so its gradient arrives first and is the buffer autograd
    sums the other into (in place when nothing else holds it).  The noted maximum then no longer describes the tensor: the data
    gradient of y0's producer must not take its f16 scale from it (a 100x too large scale saturates the split at +-6e4)."""
    from awm_amd import ops
    calls = {"from_max": 0, "versions": []}
    o_fm, o_of = M.lib.wm_gscale_from_max, ops.gscale_of

    def spy_fm(*a):
        calls["from_max"] += 1
        return o_fm(*a)

    def spy_of(g, *a):
        calls["versions"].append(g._version)
        return o_of(g, *a)
    x = rnd(2, 32, 500, seed=91)
    w0, b0 = rnd(48, 32, 3, seed=92, scale=0.1), rnd(48, seed=93)
    w1, b1 = rnd(32, 48, 3, seed=94, scale=0.1), rnd(32, seed=95)
    r1, r2 = rnd(2, 32, 500, seed=96), rnd(2, 48, 500, seed=97)
    xr = x.double().requires_grad_()
    y0r = F.conv1d(xr, w0.double(), b0.double(), padding=1)
    lb = ((y0r * 100.0) * r2.double()).sum()
    la = (F.conv1d(y0r, w1.double(), b1.double(), padding=1) * r1.double()).sum()
    (lb + la).backward()
    xd = x.to(DEV).requires_grad_()
    p = [t.to(DEV).requires_grad_() for t in (w0, b0, w1, b1)]
    y0 = M.ConvFn.apply(xd, p[0], p[1], 1, 1, 0, None, None, None)
    lb = ((y0 * 100.0) * r2.to(DEV)).sum()                   # created first: its gradient arrives second
    la = (M.ConvFn.apply(y0, p[2], p[3], 1, 1, 0, None, None, None) * r1.to(DEV)).sum()
    monkeypatch.setattr(M.lib, "wm_gscale_from_max", spy_fm)
    monkeypatch.setattr(ops, "gscale_of", spy_of)
    (lb + la).backward()
    print("gscale_of input versions", calls["versions"], "wm_gscale_from_max calls", calls["from_max"],
          "(version > 0: autograd accumulated in place)")
    check_elementwise(xd.grad, xr.grad, "upstream dx")
    assert calls["from_max"] == 0, "a gradient scale was taken from a maximum noted before the tensor was accumulated into"
