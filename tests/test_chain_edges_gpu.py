"""mlp_chain_kernel (csrc/mlp_gemm.hip) alone at its tile, strip, scene and epilogue edges: every case is ONE
s4g_mlp_gemm_f32 call into a guarded buffer (tests/chain_ref.GuardedOut: sentinel guards in front and behind, sentinel
columns on both sides of every row), compared position by position with the float64 restatement of the layers
(`nn_utils/conv.py:24-34,64-74`, the max over neighbours of `pointnet2_utils/modules.py:242-243`) -- the bf16 form with
the restatement rounded where it rounds -- relative to the row's TILE scale, and prints its worst error next to the
bound.  The bounds are the project's (tests/test_fused_gpu.py, tests/test_bf16_chain_gpu.py): f16x2 3e-5, 4e-5 with
three layers or a deep first layer; bf16 max 2e-3 / mean 2e-5 (3e-5 behind the MLP1 loaders) and 5e-2 against float64.
tests/test_chain_ref.py shows on the CPU that these very inputs catch eleven wiring errors by >= 100 x the bounds.

Families: (a) row ladder, STORE; (b) centroid ladder, MAX, every loader; (c) final-width ladder; (d) groups;
(e) scenes inside and across tiles, out_amax pinned from both sides, bit-identity of a scene; (f) ReLU flags;
(g) distinct-row MAX; (h) s4g_gemm_chain_supported against the dispatch."""
import copy

import pytest
import torch

from tests import chain_ref as R
from tests.chain_ref import BF16, F16X2, GADD, GIDX, IADD, MAX, PLAIN, REL4, STORE, STRIP, TILE
from tests.heads_ref import SCENE_SHAPES

pytestmark = pytest.mark.gpu
PRECS = [F16X2, BF16]
PNAME = {F16X2: "f16x2", BF16: "bf16"}


def _check(pr, go, what):
    go.check()
    res = R.compare(pr, go.values(), what)
    for name, (worst, bound) in res.items():
        assert worst < bound, (what, name, worst, bound)
    return res


def _run(dev, pr, what, **over):
    from s4g_release_amd import _cabi
    rc, go = R.launch(pr, dev, **over)
    _cabi.check(rc, what)
    _check(pr, go, what)
    return go


# ------------------------------------------------------------------------------------------------- (a) row ladder, STORE

ROWS = {(F16X2, 128): [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257],
        (F16X2, 256): [1, 31, 32, 33, 63, 64, 65, 129],
        (F16X2, 512): [1, 31, 32, 33, 63, 64, 65, 129],
        (BF16, 128): [1, 127, 128, 129, 255, 256, 257, 513],
        (BF16, 256): [1, 63, 64, 65, 127, 128, 129, 257],
        (BF16, 512): [1, 63, 64, 65, 127, 128, 129, 257]}
# the chain forms the ladder walks: (widths behind the first layer as multiples of C, first-layer depth / C)
FORMS = {"pair": ((1,), 1), "tri": ((1, 1), 1), "deep512": ((1,), 2), "deep1024": ((1,), 4)}
LADDER = [(p, C, "pair", P) for (p, C), rows in ROWS.items() for P in rows] + \
         [(p, 256, f, P) for f in ("tri", "deep512", "deep1024") for p in PRECS for P in ROWS[(p, 256)]]


@pytest.mark.parametrize("precision,C,form,P", LADDER)
def test_a_row_ladder_store(dev, precision, C, form, P):
    w, kc = FORMS[form]
    pr = R.problem(PLAIN, precision, C, tuple(C * x for x in w), STORE, 1, P, K1=kc * C)
    _run(dev, pr, "a %s C=%d %s P=%d" % (PNAME[precision], C, form, P))


@pytest.mark.parametrize("precision", PRECS)
def test_a_no_rows_is_ok_and_writes_nothing(dev, precision):
    pr = R.problem(PLAIN, precision, 128, (128,), STORE, 1, 1)
    rc, go = R.launch(pr, dev, P=0)
    assert rc == 0 and go.untouched()


# ----------------------------------------------------------------------------------------------- (b) centroid ladder, MAX

SCENES_OF = {1: (1, 1), 2: (2, 1), 3: (3, 1), 4: (2, 2), 5: (1, 5), 9: (3, 3)}     # nc -> (B, M): scene boundaries inside tiles
B_CASES = [(p, PLAIN, "", C) for p in PRECS for C in (128, 256, 512)] + \
          [(p, REL4, "1", C) for p in PRECS for C in (128, 256)] + [(F16X2, REL4, "0", C) for C in (128, 256)] + \
          [(p, GIDX, "", C) for p in PRECS for C in (128, 256)] + [(p, GADD, "", C) for p in PRECS for C in (128, 256, 512)]


@pytest.mark.parametrize("nc", [1, 2, 3, 4, 5, 9])
@pytest.mark.parametrize("precision,loader,mfma,C", B_CASES)
def test_b_centroid_ladder_max(dev, monkeypatch, precision, loader, mfma, C, nc):
    """K = 64, P = 64 nc.  rel_xyz4 in both S4G_MLP1_MFMA modes (the f16x2 form's phase 0 on the matrix cores or the
    vector-ALU loader; the single-plane form has the one loader and runs once); GATHER_ADD: the f16x2 dispatch takes LOAD_ADD_MFMA0,
    bf16 keeps the vector-ALU loader."""
    if mfma:
        monkeypatch.setenv("S4G_MLP1_MFMA", mfma)
    B, M = (1, nc) if loader == PLAIN else SCENES_OF[nc]
    pr = R.problem(loader, precision, C, (STRIP[C],), MAX, B, M)
    _run(dev, pr, "b %s %s%s C=%d nc=%d" % (PNAME[precision], loader, mfma and "/mfma" + mfma, C, nc))


# ------------------------------------------------------------------------------------------------ (c) final-width ladder

def _widths(C):
    S = STRIP[C]
    return sorted({64, S - 64, S, S + 64, 2 * S, 2 * S + 64})


C_CASES = [(C, co, tri, 1, epi) for C in (128, 256, 512) for co in _widths(C) for tri in (False, True)
           for epi in (STORE, MAX)] + \
          [(256, co, False, 4, STORE) for co in _widths(256)]     # ... and behind a first layer four panels deep (STORE only)


@pytest.mark.parametrize("C,cout,tri,kc,epi", C_CASES)
@pytest.mark.parametrize("precision", PRECS)
def test_c_final_width_ladder(dev, precision, C, cout, tri, kc, epi):
    """active0, the `break` on a partial strip, wnext and nn < CoutF: STORE at P = TILE + 1, MAX at three centroids."""
    n = TILE[(precision, C)] + 1 if epi == STORE else 3
    pr = R.problem(PLAIN, precision, C, (C, cout) if tri else (cout,), epi, 1, n, K1=kc * C)
    _run(dev, pr, "c %s C=%d Cout=%d %s kc=%d epi=%d" % (PNAME[precision], C, cout, "tri" if tri else "pair", kc, epi))


# ------------------------------------------------------------------------------------------------------------ (d) groups

@pytest.mark.parametrize("groups", [1, 2, 5])
@pytest.mark.parametrize("C", [256, 128])
@pytest.mark.parametrize("precision", PRECS)
def test_d_groups(dev, precision, C, groups):
    """a_gcol, c_gcol, w_gstride and b_gstride all set; every group's block against its own weights."""
    pr = R.problem(PLAIN, precision, C, (C,), STORE, 1, TILE[(precision, C)] + 1, groups=groups)
    _run(dev, pr, "d %s C=%d groups=%d" % (PNAME[precision], C, groups))


# --------------------------------------------------------------------------------- (e) scenes inside and across tiles

def _amax_pins(pr, go, out_amax, what):
    """slot_max(s) >= max |out rows of s| (smaller overflows the next layer's fp16 planes) and <= the maximum over all
    rows of every tile that touches s, joined with what rows past P produce (larger costs the next layer precision).
    The upper bound comes from the REFERENCE; its slack is the case's own error bound at that magnitude."""
    out, ref = go.values().detach().cpu(), R.reference_cached(pr, False)
    scene, tile = R.row_geometry(pr)
    slot = out_amax.cpu().amax(dim=1).double()
    nt = int(tile.max()) + 1
    tmax = torch.zeros(nt, dtype=torch.float64).scatter_reduce(0, tile, ref.abs().amax(dim=1), "amax")
    tmax[-1] = max(float(tmax[-1]), R.pad_row_value(pr))
    bd = R.bounds(pr.precision, 1 + len(pr.widths), pr.K1 > pr.C)["max"]
    worst_lo, worst_hi = 0.0, 0.0
    for s in range(pr.B):
        mine = scene == s
        lower = float(out[mine].abs().max())
        upper = float(tmax[tile[mine].unique()].max())
        assert float(slot[s]) >= lower, (what, s, float(slot[s]), lower)
        assert float(slot[s]) <= upper + bd * max(1.0, upper), (what, s, float(slot[s]), upper)
        worst_lo, worst_hi = max(worst_lo, lower / float(slot[s])), max(worst_hi, float(slot[s]) / max(upper, 1e-30))
    print("%s out_amax: out / slot <= %.6f, slot / tile bound <= %.6f" % (what, worst_lo, worst_hi))


E_CASES = [(PLAIN, C, 0, True) for C in (128, 256)] + [(IADD, 256, N2, dense) for N2 in (3, 40) for dense in (True, False)]


@pytest.mark.parametrize("B,N", SCENE_SHAPES)
@pytest.mark.parametrize("loader,C,N2,dense", E_CASES)
@pytest.mark.parametrize("precision", PRECS)
def test_e_scenes_inside_and_across_tiles(dev, precision, loader, C, N2, dense, B, N):
    """rows_per_scene = N, magnitudes cycling per scene, a_amax rows holding the true per-scene maxima; the f16x2 form's
    out_amax rows are pinned from both sides (the single-plane form has no scales and ignores them)."""
    pr = R.problem(loader, precision, C, (C,), STORE, B, N, N2=N2 or 40, dense=dense)
    what = "e %s %s C=%d N2=%d dense=%d B=%d N=%d" % (PNAME[precision], loader, C, N2, dense, B, N)
    out_amax = torch.zeros(B, 64, device=dev)
    go = _run(dev, pr, what, out_amax=out_amax)
    if precision == F16X2:
        _amax_pins(pr, go, out_amax, what)
    else:
        assert not out_amax.any()


def _with_scene0_of(dst, src):
    """dst's launch with src's layers and src's scene 0 in front of dst's other scenes."""
    pr = copy.deepcopy(dst)
    pr.Ws, pr.bs = src.Ws, src.bs
    for name in [n for n in dir(pr) if n.startswith(("_w_", "_ref_"))]:
        delattr(pr, name)
    if pr.loader == PLAIN:
        pr.A[:pr.rps] = src.A[:pr.rps]
        pr.amax = R._slots(pr.A, pr.B, 5)
    else:
        pr.S[:pr.N2], pr.nidx[0], pr.nw[0], pr.lbias = src.S[:pr.N2], src.nidx[0], src.nw[0], src.lbias
        pr.amax = R._slots(pr.S, pr.B, 9)
        if pr.dense is not None:
            pr.dense[:pr.rps] = src.dense[:pr.rps]
            pr.amax2 = R._slots(pr.dense, pr.B, 1)
        pr.floor = src.floor
    return pr


@pytest.mark.parametrize("precision,loader,C,N", [(p, l, C, N) for p in PRECS for l, C in ((PLAIN, 128), (PLAIN, 256), (IADD, 256))
                                                  for N in (128, 256) if N % TILE[(p, C)] == 0])
def test_e_a_scene_does_not_depend_on_the_other_scenes(dev, precision, loader, C, N):
    """Where TILE divides N a scene's results are bit-identical whatever the other scenes hold."""
    a = R.make_problem(loader, precision, C, [C], STORE, 2, N, seed=1)
    b = _with_scene0_of(R.make_problem(loader, precision, C, [C], STORE, 2, N, seed=2, scene_mags=(1.0, 0.02)), a)
    assert not torch.equal(a.amax[1], b.amax[1])
    what = "e' %s %s C=%d N=%d" % (PNAME[precision], loader, C, N)
    ga, gb = _run(dev, a, what), _run(dev, b, what + " (other scene replaced)")
    assert torch.equal(ga.values()[:N], gb.values()[:N])
    assert not torch.equal(ga.values()[N:], gb.values()[N:])


# -------------------------------------------------------------------------------------------------------- (f) ReLU flags

FLAGS3 = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
FLAGS2 = [(a, b) for a in (0, 1) for b in (0, 1)]


@pytest.mark.parametrize("relus", FLAGS3)
@pytest.mark.parametrize("precision", PRECS)
def test_f_relu_flags_three_layer_store(dev, precision, relus):
    pr = R.problem(PLAIN, precision, 256, (256, 256), STORE, 1, TILE[(precision, 256)] + 1, relus=relus)
    _run(dev, pr, "f %s tri STORE relus=%s" % (PNAME[precision], relus))


@pytest.mark.parametrize("relus", FLAGS2)
@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("epi", [STORE, MAX])
def test_f_relu_flags_two_layer_f16x2(dev, epi, C, relus):
    """MAX without a final ReLU runs the generic max epilogue (the maximum of signed values)."""
    pr = R.problem(PLAIN, F16X2, C, (C,), epi, 1, TILE[(F16X2, C)] + 1 if epi == STORE else 3, relus=relus)
    _run(dev, pr, "f f16x2 pair epi=%d C=%d relus=%s" % (epi, C, relus))


@pytest.mark.parametrize("relus", FLAGS2)
@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("epi", [STORE, MAX])
def test_f_relu_flags_two_layer_bf16(dev, epi, C, relus):
    """The single-plane form has no max epilogue for signed values (its waves own four row blocks): MAX without a final
    ReLU must be refused -- never S4G_OK with the output left as it was."""
    from s4g_release_amd import _cabi
    pr = R.problem(PLAIN, BF16, C, (C,), epi, 1, TILE[(BF16, C)] + 1 if epi == STORE else 3, relus=relus)
    what = "f bf16 pair epi=%d C=%d relus=%s" % (epi, C, relus)
    rc, go = R.launch(pr, dev)
    if rc != 0:
        print("%s refused: %d" % (what, rc))
        assert epi == MAX and not relus[1], (what, rc)       # the one documented refusal
        assert rc == _cabi.S4G_EUNSUPPORTED and go.untouched()
    else:
        _check(pr, go, what)


# ------------------------------------------------------------------------------------------------ (g) distinct-row MAX

@pytest.mark.parametrize("rps", [256, 512])
@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("precision,mfma", [(F16X2, "1"), (F16X2, "0"), (BF16, "1")])
def test_g_distinct_row_max(dev, monkeypatch, precision, mfma, C, rps):
    """seg4 / seg_rows layouts built by hand (tests/chain_ref.seg_problem): the reference is the maximum over each output
    row's own rows; rows no group names stay 0; rows behind seg_rows hold NaN and must not be read."""
    from s4g_release_amd import _cabi
    monkeypatch.setenv("S4G_MLP1_MFMA", mfma)
    pr = R.seg_problem(precision, C, 2 * C, rps)
    what = "g %s/mfma%s C=%d rps=%d" % (PNAME[precision], mfma, C, rps)
    rc, go = R.launch(pr, dev, zero_payload=True, seg4=pr.seg4.to(dev), seg_rows=pr.seg_rows.to(dev))
    _cabi.check(rc, what)
    go.check()
    out = go.values().detach().cpu()
    named = torch.zeros(pr.out_rows, dtype=torch.bool)
    named[pr.owner[pr.owner >= 0].unique()] = True
    assert not out[~named].any(), what + ": an output row no group names was written"
    assert named.sum() < pr.out_rows
    bd = R.bounds(precision, 2, mlp1=True)
    ref = R.seg_reference(pr, rounded=precision == BF16)
    err = R.rel_err(out, ref, pr)
    print("%s max %.3e / %.1e  mean %.3e" % (what, float(err.max()), bd["max"], float(err.mean())))
    assert float(err.max()) < bd["max"]
    if precision == BF16:
        assert float(err.mean()) < bd["mean"]
        assert float(R.rel_err(out, R.seg_reference(pr), pr).max()) < bd["exact"]


# --------------------------------------------------------------------------------------------- (h) query versus dispatch

def _h_problem(loader, precision, epi, C, K1):
    kind = {0: PLAIN, 1: GADD, 2: IADD, 3: REL4, 4: GADD, 5: IADD}[loader]
    P = 64 if epi == MAX else 65
    if kind == IADD and epi == MAX:          # a row per point, 64 points: one output row if it were accepted
        pr = R.make_problem(kind, precision, C, [C], STORE, 1, P, K1=K1, seed=loader)
        pr.epi, pr.out_rows = MAX, 1
    elif kind in (GADD, REL4) and epi == STORE:      # two centroids' rows, 65 of them used: 65 output rows if accepted
        pr = R.make_problem(kind, precision, C, [C], MAX, 1, 2, K1=K1, seed=loader)
        pr.epi, pr.P, pr.out_rows = STORE, P, P
    else:
        pr = R.make_problem(kind, precision, C, [C], epi, 1, 1 if epi == MAX else P, K1=K1, seed=loader)
    over = {}
    if loader == 1:                  # the plain GATHER loader on the same tensors: [feat | xyz] columns
        over = dict(loader=1)
    elif loader == 2:                # the plain INTERP loader: [interpolated | dense] columns
        over = dict(loader=2, C1=0)
    pr.native = pr.epi == epi and kind == {0: PLAIN, 3: REL4, 4: GADD, 5: IADD}.get(loader)
    return pr, over


@pytest.mark.parametrize("epi", [STORE, MAX])
@pytest.mark.parametrize("loader", range(6))
@pytest.mark.parametrize("precision", PRECS)
def test_h_query_matches_dispatch(dev, precision, loader, epi):
    """For every chain width and first-layer depth: a one-tile launch with W2_f16x2_frag set is accepted -- and correct --
    exactly when s4g_gemm_chain_supported says 1 (MAX with the dispatch's documented K = 64 and P % 64 == 0)."""
    from s4g_release_amd import _cabi
    lib = _cabi.lib()
    for C in (64, 128, 256, 512, 1024):
        for kc in (1, 2, 4):
            pr, over = _h_problem(loader, precision, epi, C, kc * C)
            want = lib.s4g_gemm_chain_supported(loader, epi, C, kc * C)
            what = "h %s loader=%d epi=%d C=%d Kpad16=%d query=%d" % (PNAME[precision], loader, epi, C, kc * C, want)
            rc, go = R.launch(pr, dev, **over)
            if want:
                assert pr.native, what       # (the reference below restates these loaders only)
                _cabi.check(rc, what)
                _check(pr, go, what)
            else:
                print("%s refused: %d" % (what, rc))
                assert rc in (_cabi.S4G_EINVAL, _cabi.S4G_EUNSUPPORTED) and go.untouched(), (what, rc)
