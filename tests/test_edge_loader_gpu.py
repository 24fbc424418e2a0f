"""GPU: the per-centroid bias of the add-loaders (`s4g_gemm_desc_t.cbias`, csrc/mlp_gemm.hip) at the kernels' edges.
Every case is ONE launch through the C ABI into guarded buffers (tests/chain_ref.GuardedOut).

The exact family: F, xyz, the weights and `cbias` are small integers, `cbias` row r the constant 8 r + 1 in
channel-dependent sign.  Every intermediate is then an integer every precision holds exactly (the comments at `problem`
count the bits), so the correct result is exact and a bias row taken from any other centroid shows bit for bit.  The
`cbias` rows sit inside NaN padding: a read one row off is a NaN.

  chain form   f16x2, K = 64, C = 128 / 256 / 512: the matrix-core phase 0 (`LOAD_ADD_MFMA0_CB`) -- one, two, three
               centroids, a tile that holds the last centroid of one scene and the first of the next, a tile tail
               past P; the single-plane bf16 chain, which keeps the vector-ALU loader
  vector form  `ALoader<LOAD_GATHER_ADD_CB>` in the tiled fp32 / bf16x3 / f16x2 kernels, STORE and MAX, K = 16 / 32 / 64
               (a 128-row tile holds 8 / 4 / 2 centroids), P no multiple of the tile, Cin = 4 / 36 / 128
and, on random data, the ties to the pinned form (NULL, and the bias broadcast to every row), the refusals, the f16x2
bound with a dominant `cbias`, and the distance from float64."""
import types

import pytest
import torch

from tests import chain_ref as CR

pytestmark = pytest.mark.gpu
FP32, BF16X3, BF16, F16X2 = 0, 1, 2, 3
STORE, MAX = 0, 1
GADD = 4
NPTS = 24
S4G_EINVAL = -1


def problem(B, M, K, Cin, Cout, Cout2=0, exact=True, select1=False, seed=0, cb_mag=1.0):
    """One GATHER_ADD launch's tensors on the CPU (float32 tensors; float64 copies for the reference).

    exact: integers.  |F| <= 4, |rel| <= 2 with xyz weights in {-1, 0, 1} (|w . rel| <= 6), cbias up to 8 (B M - 1) + 1
    <= 113: the loader's rows are integers <= 123 (exact in bf16's 8 bits).  W in {-1, 0, 1}: a layer's sums stay below
    Cin x 123 + 2 < 2^16 (C = 512) -- exact in fp32 accumulation, in the three bf16 planes and in the two fp16 planes
    (22 bits).  The chain's second layer (and, select1, its first: the single-plane bf16 form rounds the hidden
    activations to 8 bits) is a signed selection of two (one) inputs."""
    g = torch.Generator().manual_seed(7919 * seed + 131 * B + 17 * M + K + 3 * Cin + Cout)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()     # noqa: E731
    pb = types.SimpleNamespace(B=B, M=M, K=K, Cin=Cin, Cout=Cout, Cout2=Cout2, P=B * M * K, R=B * M)
    if exact:
        pb.xyz = ri(-1, 1, B, 3, NPTS)
        pb.F = ri(-4, 4, B * NPTS, Cin)
        pb.w1 = torch.cat([ri(-1, 1, Cin, 3), ri(-2, 2, Cin, 1)], dim=1)
        sign = torch.where(torch.arange(Cin) % 2 == 0, 1.0, -1.0)
        pb.cbias = (8.0 * torch.arange(pb.R).float() + 1.0)[:, None] * sign[None, :]
        pb.W, pb.b = ri(-1, 1, Cout, Cin), ri(-2, 2, Cout)
        if select1:
            pb.W = torch.zeros(Cout, Cin)
            pb.W[torch.arange(Cout), torch.randint(0, Cin, (Cout,), generator=g)] = ri(0, 1, Cout) * 2 - 1
    else:
        r = lambda *s: torch.randn(*s, generator=g)                                # noqa: E731
        pb.xyz = torch.rand(B, 3, NPTS, generator=g) * 0.2
        pb.F = r(B * NPTS, Cin)
        pb.w1 = r(Cin, 4)
        pb.cbias = r(pb.R, Cin) * cb_mag
        pb.W, pb.b = r(Cout, Cin) / Cin ** 0.5, r(Cout)
    cidx = torch.randint(0, NPTS, (B, M), generator=g)
    pb.ctr = torch.stack([pb.xyz[b][:, cidx[b]] for b in range(B)]).contiguous()
    pb.gidx = torch.randint(0, NPTS, (B, M, K), generator=g).int()
    rel = torch.stack([pb.xyz[b][:, pb.gidx[b].long()] - pb.ctr[b][:, :, None] for b in range(B)])   # fp32, one rounding
    pb.rel = rel.permute(0, 2, 3, 1).reshape(pb.P, 3).contiguous()
    if Cout2:
        if exact:
            pb.W2 = torch.zeros(Cout2, Cout)
            for _ in range(2):
                pb.W2[torch.arange(Cout2), torch.randint(0, Cout, (Cout2,), generator=g)] = ri(0, 1, Cout2) * 2 - 1
            pb.b2 = ri(-2, 2, Cout2)
        else:
            pb.W2, pb.b2 = torch.randn(Cout2, Cout, generator=g) / Cout ** 0.5, torch.randn(Cout2, generator=g)
    return pb


def loader_rows64(pb, cbias=None):
    """relu(F[b N + j] + W_xyz . rel + cbias[b M + m]) in float64, (P, Cin); cbias: other rows (sabotage) or None."""
    cb = (pb.cbias if cbias is None else cbias).double()
    rows = torch.cat([pb.F.view(pb.B, NPTS, pb.Cin)[b][pb.gidx[b].long().reshape(-1)] for b in range(pb.B)]).double()
    a = rows + pb.rel.double() @ pb.w1[:, :3].double().t() + cb.repeat_interleave(pb.K, dim=0)
    return a.clamp_min(0)


def reference64(pb, epi, cbias=None):
    h = (loader_rows64(pb, cbias) @ pb.W.double().t() + pb.b.double()).clamp_min(0)
    if pb.Cout2:
        h = (h @ pb.W2.double().t() + pb.b2.double()).clamp_min(0)
    return h.view(-1, pb.K, h.shape[1]).amax(dim=1) if epi == MAX else h


def _slots(x, B, slot):
    return CR._slots(x, B, slot)


def fields(pb, dev, prec, epi, go, *, cbias="own", w1=None, amax2=True):
    """The descriptor of the launch as chain_ref.call takes it.  cbias: "own" (pb.cbias inside NaN padding), None, or a
    device tensor."""
    from s4g_release_amd.fused import _Layer, _pad_k
    up = lambda x: x.to(dev).contiguous()                                          # noqa: E731
    l1 = _Layer(_pad_k(up(pb.W)), up(pb.b), pb.Cin)
    relmax = float(pb.rel.abs().max())
    kw = dict(loader=GADD, epilogue=epi, groups=1, relu=1, P=pb.P, Cin=pb.Cin, Kpad=l1.kpad, Cout=pb.Cout, W=l1.W,
              bias=l1.bias, w_gstride=pb.Cout * l1.kpad, b_gstride=pb.Cout, gidx=up(pb.gidx), feat=up(pb.F),
              xyz=up(pb.xyz), ctr=up(pb.ctr), Cf=pb.Cin, N=NPTS, M=pb.M, K=pb.K, out=go.out, ldc=go.ldc,
              c_coff=go.c_coff, c_gcol=0, precision=prec, Kpad16=l1.kpad16, W_bf16x3=l1.W3,
              mlp1_w=up(pb.w1 if w1 is None else w1), W_f16x2=l1.Wh2, w_inv_scale=l1.w_inv_scale,
              a_amax=up(_slots(pb.F, pb.B, 17)), rows_per_scene=pb.M * pb.K,
              # the loader's own term is the xyz part alone; without cbias the bias rides in it as before
              a_amax_floor=float((pb.w1[:, :3].abs().sum(1) * max(relmax, 1e-30) +
                                  (0.0 if cbias is not None else pb.w1[:, 3].abs())).max()),
              out_amax=torch.zeros((pb.B, 64), device=dev))
    if pb.Cout2:
        l2 = _Layer(_pad_k(up(pb.W2)), up(pb.b2), pb.Cout)
        frag = (lambda l: l.Wfrag_bf16) if prec == BF16 else (lambda l: l.Wfrag)
        kw.update(W_f16x2_frag=frag(l1), W2_f16x2_frag=frag(l2), w2_inv_scale=l2.w_inv_scale, bias2=l2.bias,
                  Cout2=pb.Cout2, relu2=1)
    if isinstance(cbias, str):
        pad = torch.full((pb.R + 2, pb.Cin), float("nan"))
        pad[1:pb.R + 1] = pb.cbias
        kw["_cbias_buffer"] = up(pad)
        kw["cbias"] = kw["_cbias_buffer"][1:]
        cb_host = pb.cbias
    elif cbias is not None:
        kw["cbias"], cb_host = cbias, cbias.cpu()
    if cbias is not None and amax2:
        kw["a_amax2"] = up(_slots(cb_host[:pb.R], pb.B, 5))
    return kw


def launch(pb, dev, prec, epi, floor=None, **kw):
    rows = pb.R if epi == MAX else pb.P
    go = CR.GuardedOut(dev, rows, pb.Cout2 or pb.Cout)
    f = fields(pb, dev, prec, epi, go, **kw)
    keep = f.pop("_cbias_buffer", None)               # (the padded allocation outlives the call)
    if floor is not None:
        f["a_amax_floor"] = floor
    rc = CR.call(f)
    del keep
    return rc, go


def _check_exact(pb, dev, prec, epi):
    rc, go = launch(pb, dev, prec, epi)
    assert rc == 0, rc
    go.check()
    got = go.values().cpu()
    want = reference64(pb, epi)
    assert float(want.abs().max()) < 2 ** 22                          # the family's exactness argument holds
    assert torch.equal(got.double(), want), (got.double() - want).abs().max()
    return got


# --------------------------------------------------------------------------------------------------- chain form
CHAIN_SCENES = [(1, 1), (1, 2), (1, 3), (2, 3), (3, 5)]       # (B, M): one wave; two row-waves; a half tile tail at
#                                                               C = 128; scene 0's last centroid beside scene 1's first
#                                                               (rows 128..255 at C = 128); a tile tail past P


@pytest.mark.parametrize("C", [128, 256, 512])
@pytest.mark.parametrize("B,M", CHAIN_SCENES)
def test_chain_form_takes_each_centroids_own_row(dev, C, B, M):
    pb = problem(B, M, 64, C, C, Cout2=64)
    got = _check_exact(pb, dev, F16X2, MAX)
    if pb.R > 1:
        # a bias row taken from the NEXT centroid (across the scene boundary too) gives another result at every row
        shifted = reference64(pb, MAX, torch.roll(pb.cbias, -1, dims=0))
        assert all(not torch.equal(got[r].double(), shifted[r]) for r in range(pb.R))
    if C == 128 and pb.R > 1:
        # the two row-waves of the first 128-row tile (centroids 0 and 1) carried different channel operands: with
        # either wave's row in BOTH waves the tile's result is another one
        for r in (0, 1):
            same = pb.cbias.clone()
            same[:2] = pb.cbias[r]
            one_row = reference64(pb, MAX, same)
            assert not torch.equal(got[:2].double(), one_row[:2])
            assert torch.equal(got[r].double(), one_row[r])


@pytest.mark.parametrize("C,B,M", [(128, 2, 3), (256, 3, 5)])
def test_single_plane_bf16_chain(dev, C, B, M):
    """The bf16 chain keeps the vector-ALU loader (`LOAD_GATHER_ADD_CB`, one plane): a tile of 256 / 128 rows."""
    _check_exact(problem(B, M, 64, C, C, Cout2=64, select1=True), dev, BF16, MAX)


# -------------------------------------------------------------------------------------------------- vector form
@pytest.mark.parametrize("prec", [FP32, BF16X3, F16X2], ids=["fp32", "bf16x3", "f16x2"])
@pytest.mark.parametrize("epi", [STORE, MAX], ids=["store", "max"])
@pytest.mark.parametrize("K,B,M", [(16, 2, 5), (32, 2, 3), (64, 1, 3)])           # P = 160 / 192 / 192: a tile tail
@pytest.mark.parametrize("Cin", [4, 36, 128])
def test_tiled_kernels_take_each_centroids_own_row(dev, prec, epi, K, B, M, Cin):
    pb = problem(B, M, K, Cin, 40)
    assert pb.P % 128
    got = _check_exact(pb, dev, prec, epi)
    shifted = reference64(pb, epi, torch.roll(pb.cbias, -1, dims=0))
    assert not torch.equal(got.double(), shifted)


# ------------------------------------------------------------------------------- ties to the form without cbias
FORMS = [("chain128", F16X2, MAX, dict(B=2, M=3, K=64, Cin=128, Cout=128, Cout2=64)),
         ("chain512", F16X2, MAX, dict(B=1, M=3, K=64, Cin=512, Cout=512, Cout2=64)),
         ("bf16chain", BF16, MAX, dict(B=2, M=3, K=64, Cin=128, Cout=128, Cout2=64)),
         ("fp32", FP32, STORE, dict(B=2, M=5, K=16, Cin=36, Cout=40)),
         ("bf16x3", BF16X3, MAX, dict(B=2, M=3, K=32, Cin=36, Cout=40)),
         ("f16x2", F16X2, STORE, dict(B=2, M=5, K=16, Cin=36, Cout=40))]


@pytest.mark.parametrize("name,prec,epi,shape", FORMS, ids=[f[0] for f in FORMS])
def test_null_and_broadcast_bias_give_the_pinned_forms_bits(dev, name, prec, epi, shape):
    """cbias = NULL: the launch as it always was (mlp1_w[].w is the bias).  cbias = that bias broadcast to every row,
    mlp1_w[].w then garbage: the same bits -- the new form computes what the pinned one does."""
    pb = problem(exact=False, seed=3, **shape)
    rc0, go0 = launch(pb, dev, prec, epi, cbias=None)
    assert rc0 == 0
    go0.check()
    bcast = pb.w1[:, 3][None, :].expand(pb.R, -1).contiguous().to(dev)
    junk = pb.w1.clone()
    junk[:, 3] = 777.0
    # f16x2: the activation scale follows the bound, so the second launch is given the first one's -- F's maxima plus
    # a floor with the bias in it, no a_amax2
    floor0 = float((pb.w1[:, :3].abs().sum(1) * float(pb.rel.abs().max()) + pb.w1[:, 3].abs()).max())
    rc1, go1 = launch(pb, dev, prec, epi, cbias=bcast, w1=junk, amax2=False, floor=floor0)
    assert rc1 == 0
    go1.check()
    assert torch.equal(go0.values().view(torch.int32), go1.values().view(torch.int32))


# ------------------------------------------------------------------------------------------------------ refusals
def _plain_fields(dev, go, P=64, C=8):
    from s4g_release_amd.fused import _Layer, _pad_k
    l = _Layer(_pad_k(torch.randn(8, C, device=dev)), torch.randn(8, device=dev), C)
    return dict(loader=0, epilogue=STORE, groups=1, relu=1, P=P, Cin=C, Kpad=l.kpad, Cout=8, W=l.W, bias=l.bias,
                w_gstride=8 * l.kpad, b_gstride=8, out=go.out, ldc=go.ldc, c_coff=go.c_coff, precision=FP32,
                Kpad16=l.kpad16, W_bf16x3=l.W3, W_f16x2=l.Wh2, w_inv_scale=l.w_inv_scale, _layer=l)


@pytest.mark.parametrize("loader", ["plain", "gather_mlp1", "interp_add", "misaligned"])
def test_cbias_is_refused_where_it_has_no_meaning(dev, loader):
    """A descriptor the library ACCEPTS without cbias answers S4G_EINVAL with it, outputs and guards untouched."""
    P, C = 64, 8
    go = CR.GuardedOut(dev, P, 8)
    cb = torch.zeros((P, C), device=dev)
    if loader == "misaligned":
        pb = problem(1, 4, 16, C, 8)
        f = fields(pb, dev, FP32, STORE, go)
        buf = f.pop("_cbias_buffer")
        good = dict(f)
        f["cbias"] = buf.view(-1)[C + 1:]                 # 4 bytes past a row start
    else:
        f = _plain_fields(dev, go, P, C)
        keep = f.pop("_layer")                            # noqa: F841
        if loader == "plain":
            f.update(A=torch.randn(P, C, device=dev), lda=C)
        elif loader == "gather_mlp1":
            f.update(loader=3, gidx=torch.zeros(P, dtype=torch.int32, device=dev), xyz=torch.rand(1, 3, 5, device=dev),
                     ctr=torch.rand(1, 3, 4, device=dev), N=5, M=4, K=16, mlp1_w=torch.randn(C, 4, device=dev))
        else:
            f.update(loader=5, nidx=torch.zeros((P, 3), dtype=torch.int32, device=dev),
                     nw=torch.full((P, 3), 1 / 3, device=dev), sparse=torch.randn(7, C, device=dev), C2=C, N1=P, N2=7,
                     loader_bias=torch.randn(C, device=dev))
        good = dict(f)
        f["cbias"] = cb
    assert CR.call(f) == S4G_EINVAL
    assert go.untouched()
    assert CR.call(good) == 0                             # ... and the same descriptor without it runs
    go.check()


# ------------------------------------------------------------------------------------------- bounds and float64
def _tile_err(pb, got, want, epi, tile):
    pr = types.SimpleNamespace(out_rows=want.shape[0], epi=epi, rps=pb.M * pb.K, tile=tile, groups=1)
    rows = torch.arange(pr.out_rows) * (pb.K if epi == MAX else 1)
    scene, tl = rows // pr.rps, rows // tile
    d = (got.double() - want).abs().reshape(want.shape[0], 1, -1) / CR.tile_scale(want, scene, tl, 1)
    return float(torch.nan_to_num(d, nan=float("inf")).max())


@pytest.mark.parametrize("name,prec,epi,shape", [f for f in FORMS if f[1] != BF16], ids=[f[0] for f in FORMS if f[1] != BF16])
def test_random_data_is_within_the_projects_bound_of_float64(dev, name, prec, epi, shape):
    pb = problem(exact=False, seed=5, **shape)
    rc, go = launch(pb, dev, prec, epi)
    assert rc == 0
    go.check()
    tile = CR.TILE[(F16X2, shape["Cout"])] if shape.get("Cout2") else 128
    e = _tile_err(pb, go.values().cpu(), reference64(pb, epi), epi, tile)
    bound = CR.bounds(F16X2, 2 if shape.get("Cout2") else 1)["max"]
    print("%s: %.3e / %.1e of the tile's scale" % (name, e, bound))
    assert e < bound


@pytest.mark.parametrize("name,prec,epi,shape", [FORMS[0], FORMS[1], FORMS[5]], ids=["chain128", "chain512", "f16x2"])
def test_f16x2_scale_follows_a_amax2(dev, name, prec, epi, shape):
    """cbias 2^10 times larger than F and the xyz term: with its maxima in a_amax2 the activation scale covers it (no
    fp16 overflow) and the result stays within the f16x2 bound; the xyz term then sits 10 bits down in the phase-0
    operand, which the bound -- a fraction of the tile's scale -- allows."""
    pb = problem(exact=False, seed=7, cb_mag=1024.0, **shape)
    rc, go = launch(pb, dev, prec, epi)
    assert rc == 0
    go.check()
    tile = CR.TILE[(F16X2, shape["Cout"])] if shape.get("Cout2") else 128
    want = reference64(pb, epi)
    e = _tile_err(pb, go.values().cpu(), want, epi, tile)
    bound = CR.bounds(F16X2, 2 if shape.get("Cout2") else 1)["max"]
    print("%s: %.3e / %.1e of the tile's scale (max |ref| %.1f)" % (name, e, bound, float(want.abs().max())))
    assert e < bound
