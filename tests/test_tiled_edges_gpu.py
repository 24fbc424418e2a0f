"""The tiled single-layer kernels behind s4g_mlp_gemm_f32 (mlp_gemm_kernel, mlp_gemm_bf16x3_kernel, mlp_gemm_f16x2_kernel
with PL = 2 / 1 and NCB = 2 / 4, csrc/mlp_gemm.hip) alone at their tile, column, depth, scene and epilogue edges: every
case is ONE s4g_mlp_gemm_f32 call into guarded buffers (tests/tiled_ref.Guard: sentinel guards in front and behind, sentinel
columns on both sides of every row, ldc > Cout, c_coff > 0; each channels-first tensor with guards around it), compared
element by element with the float64 restatement of the layer and its epilogue -- the one-plane bf16 form also with the
restatement rounded where it rounds -- relative to the element's TILE-AND-SCENE scale (tests/tiled_ref.scale), and prints
its worst error next to the bound.  W_f16x2_frag is never set, so plain layers stay on the tiled kernels without a knob.

Bounds: f16x2 and bf16x3 2e-5 (tests/test_fused_gpu.py); one-plane bf16 2e-3 max / 2e-5 mean against the rounded
restatement and 5e-2 against float64 (tests/chain_ref.bounds); fp32 MFMA 2.4e-6 = 4 x 6.0e-7, the largest distance of the
plain fp32 CPU product (torch) of these very cases from float64 at the same scale (measured 5.66e-7 over the suite's fp32
cases by tests/test_tiled_ref.py, which fails if a case exceeds the figure; the summation order differs, hence 4 x).
tests/test_tiled_ref.py shows on the CPU that these inputs catch fifteen wiring errors by >= 100 x the bounds.

Families: (a) row ladder; (b) column ladder, float4 and scalar stores; (c) depth ladder; (d) groups; (e) the 128 x 256
tile on both sides of its predicate; (f) EPI_MAX; (g) EPI_MAX_CHANNEL_FIRST; (h) EPI_CHANNEL_FIRST; (i) loaders inside a
tile; (j) scenes and scales of the f16x2 form.  The module-level case builders are what tests/test_tiled_ref.py imports."""
import pytest
import torch

from tests import tiled_ref as T
from tests.tiled_ref import (BF16, BF16X3, CF, CFIRST, F16X2, FP32, GADD, GATHER, GIDX, IADD, INTERP, MAX, MAXCF, PLAIN,
                             PNAME, PRECS_ALL, PRECS_CF, REL4, STORE)

pytestmark = pytest.mark.gpu
SPLIT = (F16X2, BF16, BF16X3)         # the precisions that walk Kpad16


def _check(pr, outs, what):
    outs.check()
    res = T.compare(pr, outs.matrix(), what)
    for name, (worst, bound) in res.items():
        assert worst < bound, (what, name, worst, bound)
    return res


def _run(dev, pr, what, layout=None, **over):
    from s4g_release_amd import _cabi
    rc, outs = T.launch(pr, dev, layout=layout, **over)
    _cabi.check(rc, what)
    _check(pr, outs, what)
    return outs


# ------------------------------------------------------------------------------------------------------ (a) row ladder

def case_a(precision, P):
    return T.problem(PLAIN, STORE, precision, 16, 40, n=P)


@pytest.mark.parametrize("P", T.ROWS)
@pytest.mark.parametrize("precision", PRECS_ALL)
def test_a_row_ladder(dev, precision, P):
    _run(dev, case_a(precision, P), "a %s P=%d" % (PNAME[precision], P))


@pytest.mark.parametrize("precision", PRECS_ALL)
def test_a_no_rows_is_ok_and_writes_nothing(dev, precision):
    rc, outs = T.launch(case_a(precision, 1), dev, P=0)
    assert rc == 0 and outs.untouched()


# --------------------------------------------------------------------------------------------------- (b) column ladder

def case_b(precision, cout):
    return T.problem(PLAIN, STORE, precision, 16, cout, n=129)


def layout_b(cout, variant):
    """base: ldc, c_coff and the pointer 4-aligned (float4 stores wherever Cout % 4 == 0); then each breaks in turn."""
    c4 = -(-cout // 4) * 4
    return {"base": {}, "ldc": dict(ldc=c4 + 9), "coff": dict(c_coff=5, ldc=c4 + 12), "ptr": dict(shift=1)}[variant]


B_CASES = [(p, c, "base") for p in PRECS_ALL for c in T.COLS] + \
          [(p, c, v) for p in (F16X2, FP32) for c in T.COLS if c % 4 == 0 for v in ("ldc", "coff", "ptr")]


@pytest.mark.parametrize("precision,cout,variant", B_CASES)
def test_b_column_ladder(dev, precision, cout, variant):
    _run(dev, case_b(precision, cout), "b %s Cout=%d %s" % (PNAME[precision], cout, variant), layout=layout_b(cout, variant))


# ---------------------------------------------------------------------------------------------------- (c) depth ladder

def case_c(precision, cin):
    """PLAIN with lda > Cin and a_coff > 0 (every PLAIN problem of tests/tiled_ref.py has both)."""
    return T.problem(PLAIN, STORE, precision, cin, 40, n=129)


def case_c_cf(precision, cin):
    return T.problem(CFIRST, STORE, precision, cin, 40, B=2, n=70)


C_CASES = [(p, cin) for p in SPLIT for _, cin in T.DEPTH16] + [(FP32, cin) for cin in T.DEPTH8]


@pytest.mark.parametrize("precision,cin", C_CASES)
def test_c_depth_ladder(dev, precision, cin):
    pr = case_c(precision, cin)
    _run(dev, pr, "c %s Cin=%d Kpad=%d Kpad16=%d" % (PNAME[precision], cin, pr.Kpad, pr.Kpad16))


@pytest.mark.parametrize("cin", [1, 3, 5, 33])
@pytest.mark.parametrize("precision", PRECS_CF)
def test_c_depth_channel_first(dev, precision, cin):
    _run(dev, case_c_cf(precision, cin), "c %s cfirst Cin=%d" % (PNAME[precision], cin))


# ----------------------------------------------------------------------------------------------------------- (d) groups

def case_d(precision, groups):
    return T.problem(PLAIN, STORE, precision, 16, 40, n=129, groups=groups)


@pytest.mark.parametrize("groups", [1, 2, 5])
@pytest.mark.parametrize("precision", PRECS_ALL)
def test_d_groups(dev, precision, groups):
    """a_gcol, c_gcol (a gap between the groups' blocks), w_gstride and b_gstride (gaps, tests/tiled_ref._weights) all
    set; every group's block against its own weights."""
    _run(dev, case_d(precision, groups), "d %s groups=%d" % (PNAME[precision], groups), layout=dict(c_gcol=44))


# -------------------------------------------------------------------------------------------------- (e) the wide tile

def case_e_plain(precision, cout, mt):
    return T.problem(PLAIN, STORE, precision, 16, cout, n=(mt - 1) * 128 + 1, groups=T.WIDE_GROUPS)


def case_e_gather(loader, epi, precision, nc):
    return T.problem(loader, epi, precision, 16, T.WIDE_GATHER_COUT, n=nc, K=64)


def case_e_split(precision, mt):
    cout, split_n, _ = T.WIDE_SPLIT
    return T.problem(PLAIN, STORE, precision, 16, cout, n=(mt - 1) * 128 + 1, split_n=split_n)


@pytest.mark.parametrize("mt", [T.WIDE_MT, T.WIDE_MT - 1])
@pytest.mark.parametrize("cout", [256] + T.WIDE_COLS)
@pytest.mark.parametrize("precision", [F16X2, BF16])
def test_e_wide_plain_store(dev, precision, cout, mt):
    """groups = 8, P = (mt - 1) 128 + 1: 32 row tiles reach 512 workgroups, 31 do not (Cout = 516 has three 256-column
    tiles and stays wide at 31: 744); Cout = 256 is never wide."""
    pr = case_e_plain(precision, cout, mt)
    _run(dev, pr, "e %s plain Cout=%d mt=%d wgs=%d wide=%d" % (PNAME[precision], cout, mt, T.wide_wgs(pr.P, cout, 8), T.wide(pr)))


E_GATHER = [(p, l, e) for p in (F16X2, BF16) for l, e in ((GIDX, MAX), (REL4, MAX), (GADD, MAX), (GADD, STORE))] + \
           [(F16X2, PLAIN, MAXCF)]          # (EPI_MAX_CHANNEL_FIRST has no one-plane form)


@pytest.mark.parametrize("nc", [T.WIDE_GATHER_NC, T.WIDE_GATHER_NC - 1])
@pytest.mark.parametrize("precision,loader,epi", E_GATHER)
def test_e_wide_gather_and_max_cf(dev, precision, loader, epi, nc):
    """Cout = 1028 (five 256-column tiles, the last 4 wide), K = 64: 205 centroids are 103 row tiles = 515 workgroups,
    204 are 102 = 510."""
    pr = case_e_gather(loader, epi, precision, nc)
    _run(dev, pr, "e %s %s epi=%d nc=%d wgs=%d wide=%d" % (PNAME[precision], loader, epi, nc, T.wide_wgs(pr.P, pr.Cout), T.wide(pr)))


@pytest.mark.parametrize("mt", [T.WIDE_SPLIT[2], T.WIDE_SPLIT[2] - 1])
@pytest.mark.parametrize("precision", [F16X2, BF16])
def test_e_wide_two_outputs(dev, precision, mt):
    pr = case_e_split(precision, mt)
    oa, oa2 = torch.zeros(1, 64, device=dev), torch.zeros(1, 64, device=dev)
    outs = _run(dev, pr, "e %s two outputs mt=%d wide=%d" % (PNAME[precision], mt, T.wide(pr)), out_amax=oa, out_amax2=oa2)
    if precision == F16X2:       # each tensor's maximum goes to its own slot row
        for g, slot in zip(outs.g, (oa, oa2)):
            lo = float(g.values().abs().max())
            assert lo <= float(slot.max()) <= lo * (1 + 1e-6) + 1e-30


# ------------------------------------------------------------------------------------------------------------ (f) EPI_MAX

def case_f(loader, precision, K, nc, relu):
    return T.problem(loader, MAX, precision, 16, 40, n=nc, K=K, relu=relu)


F_CASES = [(l, K, nc, relu) for l in (PLAIN, GATHER, GIDX, REL4, GADD) for K in (16, 32, 64)
           for nc in sorted({128 // K - 1, 128 // K, 128 // K + 1, 1, 2} - {0}) for relu in (0, 1)]


@pytest.mark.parametrize("loader,K,nc,relu", F_CASES)
@pytest.mark.parametrize("precision", PRECS_ALL)
def test_f_max(dev, precision, loader, K, nc, relu):
    _run(dev, case_f(loader, precision, K, nc, relu), "f %s %s K=%d nc=%d relu=%d" % (PNAME[precision], loader, K, nc, relu))


# --------------------------------------------------------------------------------------------- (g) EPI_MAX_CHANNEL_FIRST

G_M = {1: 129, 2: 65, 31: 5, 32: 5, 33: 4, 127: 3, 128: 2, 129: 2, 256: 2, 300: 2}     # K -> M: group ends before, on, after tile ends


def case_g(precision, K, B, cout):
    return T.problem(CFIRST if cout == 72 else PLAIN, MAXCF, precision, 16, cout, B=B, n=G_M[K], K=K)


@pytest.mark.parametrize("cout", [1, 72, 128, 129])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", sorted(G_M))
@pytest.mark.parametrize("precision", PRECS_CF)
def test_g_max_channel_first(dev, precision, K, B, cout):
    """Any K, merged across tiles by atomicMax: two runs are bit-identical and a (group, channel) whose maximum is
    negative stays exactly 0 (Cout = 72 runs the CHANNEL_FIRST loader, the others PLAIN)."""
    pr = case_g(precision, K, B, cout)
    what = "g %s K=%d B=%d M=%d Cout=%d" % (PNAME[precision], K, B, G_M[K], cout)
    first = _run(dev, pr, what)
    rc, again = T.launch(pr, dev)
    assert rc == 0 and torch.equal(first.matrix(), again.matrix()), what + ": two runs differ"
    pre = T.epilogue_pre_activation(pr)
    negative = pre < -1e-3 * T.scale(pr, T.reference_cached(pr))
    assert negative.any() and not first.matrix().cpu()[negative].any(), what


# ------------------------------------------------------------------------------------------------- (h) EPI_CHANNEL_FIRST

H_HEADS = [((21,), None), ((21,), 16), ((5, 16), 5), ((5, 16), 9), ((3, 9, 4, 5), None), ((3, 9, 4, 5), 16), ((3, 9, 4, 5), 14)]


def case_h(loader, precision, cf_N, heads, sig):
    return T.problem(loader, CF, precision, 16, 21, B=3, n=cf_N, relu=0, heads=heads, sigmoid_from=sig)


@pytest.mark.parametrize("heads,sig", H_HEADS)
@pytest.mark.parametrize("cf_N", [4, 36, 37, 128, 130])
@pytest.mark.parametrize("loader,precision", [(PLAIN, p) for p in PRECS_ALL] + [(CFIRST, p) for p in PRECS_CF])
def test_h_channel_first(dev, loader, precision, cf_N, heads, sig):
    """B = 3 scenes of cf_N points: row quads straddle a scene where cf_N % 4 != 0; one, two and four heads with uneven
    cf_start; cf_sigmoid_from absent, at a head boundary, inside a head."""
    _run(dev, case_h(loader, precision, cf_N, heads, sig),
         "h %s %s cf_N=%d heads=%s sigmoid_from=%s" % (PNAME[precision], loader, cf_N, heads, sig))


# ----------------------------------------------------------------------------------------------- (i) loaders inside a tile

def case_i_gather(precision, cf, epi=STORE):
    return T.problem(GATHER, epi, precision, cf, 40, B=4, n=5, K=16)


def case_i_family(loader, precision):
    return T.problem(loader, STORE, precision, 16, 40, B=4, n=5, K=16)


def case_i_interp(precision, c2, c1):
    return T.problem(INTERP, STORE, precision, c2, 40, B=4, n=50, C1=c1)


def case_i_iadd(precision, dense):
    return T.problem(IADD, STORE, precision, 16, 40, B=4, n=50, dense=dense)


def case_i_cfirst(precision):
    return T.problem(CFIRST, STORE, precision, 16, 40, B=4, n=37)


@pytest.mark.parametrize("epi", [STORE, MAX])
@pytest.mark.parametrize("cf", [0, 4, 28, 32, 60])
@pytest.mark.parametrize("precision", PRECS_ALL)
def test_i_gather_xyz_chunk(dev, precision, cf, epi):
    """The xyz chunk last in a K tile (Cf = 28, 60), first in the next (32), in the middle (4) and alone (0); 80 rows
    per scene, B = 4: tiles straddle one and two scene boundaries."""
    _run(dev, case_i_gather(precision, cf, epi), "i %s gather Cf=%d epi=%d" % (PNAME[precision], cf, epi))


@pytest.mark.parametrize("loader", [GIDX, REL4, GADD])
@pytest.mark.parametrize("precision", PRECS_ALL)
def test_i_gather_family_scene_boundaries(dev, precision, loader):
    _run(dev, case_i_family(loader, precision), "i %s %s 80 rows per scene" % (PNAME[precision], loader))


@pytest.mark.parametrize("c2,c1", [(4, 0), (4, 12), (36, 0), (36, 12)])
@pytest.mark.parametrize("precision", PRECS_ALL)
def test_i_interp(dev, precision, c2, c1):
    """N1 = 50 per scene, B = 4: pp / N1 changes inside a tile; C2 = 36, C1 = 12: the dense columns start inside a K tile."""
    _run(dev, case_i_interp(precision, c2, c1), "i %s interp C2=%d C1=%d" % (PNAME[precision], c2, c1))


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("precision", PRECS_ALL)
def test_i_interp_add(dev, precision, dense):
    _run(dev, case_i_iadd(precision, dense), "i %s interp_add dense=%d" % (PNAME[precision], dense))


@pytest.mark.parametrize("precision", PRECS_CF)
def test_i_channel_first_scenes(dev, precision):
    _run(dev, case_i_cfirst(precision), "i %s cfirst aL=37 B=4" % PNAME[precision])


# ------------------------------------------------------------------------------------------- (j) scenes and scales, f16x2

J_MAGS = (40.0, 0.02, 1.0)            # scenes 0 and 1 share a tile wherever tiles straddle: 2000 x apart


def case_j(loader, rps):
    if loader == IADD:
        return T.problem(IADD, STORE, F16X2, 16, 40, B=3, n=rps, scene_mags=J_MAGS)
    return T.problem(PLAIN, STORE, F16X2, 16, 40, B=3, n=rps, scene_mags=J_MAGS)


def _amax_pins(pr, outs, out_amax, what):
    """slot_max(s) >= max |out rows of s| (smaller overflows the consumer's fp16 planes) and <= the REFERENCE's maximum
    over every tile that touches s, joined with what the rows past P produce (zeros in: the activated bias), plus the
    case's own error bound at that magnitude (larger costs the consumer precision)."""
    out, ref = outs.matrix().detach().cpu(), T.reference_cached(pr)
    bm = T.geometry().GM_BM
    p = torch.arange(pr.P)
    scene, tile = p // pr.rps, p // bm
    slot = out_amax.cpu().amax(dim=1).double()
    tmax = torch.zeros(int(tile.max()) + 1, dtype=torch.float64).scatter_reduce(0, tile, ref.abs().amax(dim=1), "amax")
    if pr.P % bm:
        pad = pr.bias.double().clamp_min(0) if pr.relu else pr.bias.double().abs()
        tmax[-1] = max(float(tmax[-1]), float(pad.max()))
    bd = T.bounds(pr.precision)["max"]
    worst_lo, worst_hi = 0.0, 0.0
    for s in range(pr.B):
        mine = scene == s
        lower = float(out[mine].abs().max())
        upper = float(tmax[tile[mine].unique()].max())
        assert float(slot[s]) >= lower, (what, s, float(slot[s]), lower)
        assert float(slot[s]) <= upper + bd * max(1.0, upper), (what, s, float(slot[s]), upper)
        worst_lo, worst_hi = max(worst_lo, lower / float(slot[s])), max(worst_hi, float(slot[s]) / max(upper, 1e-30))
    print("%s out_amax: out / slot <= %.6f, slot / tile bound <= %.6f" % (what, worst_lo, worst_hi))


@pytest.mark.parametrize("rps", [64, 128, 192])
@pytest.mark.parametrize("loader", [PLAIN, IADD])
def test_j_scenes_and_out_amax(dev, loader, rps):
    """rows_per_scene inside a tile, equal to a tile, straddling; a_amax / a_amax2 rows hold the true per-scene maxima."""
    pr = case_j(loader, rps)
    what = "j f16x2 %s rows_per_scene=%d" % (loader, rps)
    out_amax = torch.zeros(pr.B, 64, device=dev)
    outs = _run(dev, pr, what, out_amax=out_amax)
    _amax_pins(pr, outs, out_amax, what)


def _beside(alone, neighbour_mag):
    """alone's scene followed by a second scene of the given magnitude (NaN: a scene of NaNs), same layer."""
    pr = T.make(PLAIN, STORE, F16X2, 16, 40, B=2, n=alone.rps, scene_mags=(1.0, 1.0), seed=5)
    pr.W, pr.bias = alone.W, alone.bias
    pr.A[:alone.rps] = alone.A
    pr.A[alone.rps:] *= neighbour_mag
    pr.amax = T._slots(pr.A, 2, 5)
    return pr


def test_j_a_scene_does_not_depend_on_its_neighbour(dev):
    """rows_per_scene = 128 = the tile: a scene alone equals the same scene in a batch bit for bit, next to a scene 2^10
    times larger and next to a NaN scene."""
    alone = T.make(PLAIN, STORE, F16X2, 16, 40, B=1, n=128, seed=4)
    ga = _run(dev, alone, "j' alone")
    big = _beside(alone, 1024.0)
    assert float(big.amax[1].max()) >= 512 * float(big.amax[0].max())
    gb = _run(dev, big, "j' beside a 2^10 x scene")
    assert torch.equal(ga.matrix(), gb.matrix()[:128])
    nan = _beside(alone, float("nan"))
    from s4g_release_amd import _cabi
    rc, gn = T.launch(nan, dev)
    _cabi.check(rc, "j' beside a NaN scene")
    assert torch.equal(ga.matrix(), gn.matrix()[:128])
    rest = gn.matrix()[128:].contiguous()
    assert (rest.view(torch.int32) != T.SENTINEL_BITS).all()      # the NaN scene's rows were written (the ReLU turns NaN into 0)
