"""CPU checks of what tests/test_tiled_edges_gpu.py stands on (tests/tiled_ref.py): the float64 restatement against
independent formulations, the geometry read from csrc/mlp_gemm.hip against the ladders, the guarded buffers' own detection,
the conditions the max / scene families' inputs must meet, the fp32 bound's yardstick, and the sabotage table -- on the GPU
tests' OWN inputs each wiring error the tiled kernels' structure makes possible must move the reference by >= 100 x the
bound the GPU case asserts (the bar of tests/test_heads_ref.py and tests/test_chain_ref.py), on at least one case of its
family, so a kernel with that error cannot pass.

Measured ratios (miss / bound, the miss relative to the element's tile-and-scene scale; inf: not finite):

    1  two 32-row blocks of a wave swapped              f16x2 a P=129                              46 000 x
    2  the last partial column tile dropped             f16x2 b Cout=129                           50 000 x
    3  bias of the neighbouring 32-column block         f16x2 b Cout=129                           31 000 x
    4  max-group boundary shifted by one row            f16x2 f plain K=16 nc=9                    13 000 x
    5  a straddling group keeps one side                f16x2 g K=300 B=3 Cout=129                 23 000 x
    6  the last half-deep K step dropped                f16x2 c Cin=48                             23 000 x
    7  GATHER's xyz columns dropped / a chunk off       f16x2 i gather Cf=28                1 400 / 22 000 x
    8  a gathered row's scene from the tile's first row f16x2 i gather Cf=28                       49 000 x
    9  the three interpolation weights rotated          f16x2 i interp C2=36 C1=12                 34 000 x
    10 LOAD_INTERP's dense columns dropped              f16x2 i interp C2=36 C1=12                 24 000 x
    11 the previous scene's activation scale            f16x2 j plain rows_per_scene=192                inf
    12 out2's column offset off by one tile             f16x2 e two outputs, 170 row tiles         50 000 x
    13 channels-first point index not reduced           f16x2 h cf_N=37, four heads                75 000 x
    14 cf_sigmoid_from one channel off                  f16x2 h cf_N=37, four heads, from 14       34 000 x
    15 head boundary cf_start one channel off           f16x2 h cf_N=37, four heads                31 000 x

(50 000 x = 1 / 2e-5: the miss is as large as the scale itself; entry 13 exceeds it where a value of the loud scene lands
in a quiet scene's place.  The figures are printed by the test; the table is rounded down to two digits.)"""
import pytest
import torch

from tests import chain_ref as CR
from tests import test_tiled_edges_gpu as G
from tests import tiled_ref as T
from tests.tiled_ref import BF16, CF, CFIRST, F16X2, FP32, GADD, GATHER, GIDX, INTERP, MAX, MAXCF, PLAIN, REL4, STORE

BAR = 100.0


# ------------------------------------------------------------------------------------------------------------ geometry

def test_geometry_is_read_from_the_source_and_the_ladders_bracket_it():
    """A moved tile size or wide-tile threshold fails here until the ladders of tests/tiled_ref.py follow."""
    g = T.geometry()
    for bm in (g.GM_BM // 4, g.GM_BM // 2, g.GM_BM):                 # 32-row block, wave, tile
        assert {bm - 1, bm, bm + 1} <= set(T.ROWS), bm
    assert 2 * g.GM_BM + 1 in T.ROWS                                  # more than two row tiles
    for bn in (32, 64, g.GM_BN, g.H2_BN[1]):                          # column block, wave, both tile widths
        assert {bn - 1, bn} <= set(T.COLS) and any(bn < c <= bn + 4 for c in T.COLS), bn
    assert g.H2_BN == [g.GM_BN, 2 * g.GM_BN] and g.H2_BK == g.GM_BK == 32
    k16 = {k for k, _ in T.DEPTH16}
    assert {g.H2_BK // 2, g.H2_BK, g.H2_BK + 16, 2 * g.H2_BK, 2 * g.H2_BK + 16} <= k16    # whole and half-deep last steps
    assert {cin for _, cin in T.DEPTH16} >= {k - 12 for k in k16} | k16
    assert {k % g.GM_BK for k in T.DEPTH8} == {0, 8, 24} and g.GM_BK + 8 in T.DEPTH8 and 2 * g.GM_BK + 8 in T.DEPTH8
    # the wide tile: both sides of Cout > WIDE_COUT and of wide_wgs >= WIDE_WGS, exactly at the threshold
    assert g.WIDE_COUT in [256] + T.WIDE_COLS and min(T.WIDE_COLS) <= g.WIDE_COUT + 4
    for cout in T.WIDE_COLS:
        hi, lo = G.case_e_plain(F16X2, cout, T.WIDE_MT), G.case_e_plain(F16X2, cout, T.WIDE_MT - 1)
        assert T.wide(hi) and hi.P % g.GM_BM == 1
        assert T.wide(lo) == (T.wide_wgs(lo.P, cout, T.WIDE_GROUPS) >= g.WIDE_WGS)
    assert T.wide_wgs(G.case_e_plain(F16X2, 260, T.WIDE_MT).P, 260, T.WIDE_GROUPS) == g.WIDE_WGS
    assert not T.wide(G.case_e_plain(F16X2, 260, T.WIDE_MT - 1)) and not T.wide(G.case_e_plain(BF16, 256, T.WIDE_MT))
    for loader, epi in ((GIDX, MAX), (REL4, MAX), (GADD, MAX), (GADD, STORE), (PLAIN, MAXCF)):
        hi, lo = (G.case_e_gather(loader, epi, F16X2, T.WIDE_GATHER_NC - d) for d in (0, 1))
        assert T.wide(hi) and not T.wide(lo)
        assert T.wide_wgs(lo.P, lo.Cout) < g.WIDE_WGS <= T.wide_wgs(hi.P, hi.Cout) < g.WIDE_WGS + 5
    hi, lo = G.case_e_split(F16X2, T.WIDE_SPLIT[2]), G.case_e_split(BF16, T.WIDE_SPLIT[2] - 1)
    assert T.wide(hi) and not T.wide(lo) and hi.split_n % g.H2_BN[1] == 0
    assert not T.wide(T.make(GATHER, STORE, F16X2, 16, 1028, n=205, K=64))       # the loaders the predicate leaves out


def test_every_dispatched_pair_has_a_builder_in_every_precision():
    """The (loader, epilogue) lists at the end of s4g_mlp_gemm_f32 against tests/tiled_ref.py's."""
    import re
    src = open(T._SRC).read()
    names = {"LOAD_PLAIN": {PLAIN}, "LOAD_GATHER": {GATHER}, "LOAD_INTERP": {INTERP}, "LOAD_GATHER_MLP1": {GIDX, REL4},
             "LOAD_GATHER_ADD": {GADD}, "LOAD_INTERP_ADD": {T.IADD}, "LOAD_CHANNEL_FIRST": {CFIRST}}
    epis = {"EPI_STORE": STORE, "EPI_MAX": MAX, "EPI_CHANNEL_FIRST": CF, "EPI_MAX_CF": MAXCF}
    for macro, mine in (("S4G_GEMM_CASE", T.PAIRS_ALL), ("S4G_GEMM_CASE_CF", T.PAIRS_CF)):
        listed = {(l, epis[e]) for L, e in re.findall(r"^  %s\((\w+), (\w+)\)$" % macro, src, re.M) for l in names[L]}
        assert listed == set(mine), macro
    for loader, epi in T.PAIRS_ALL + T.PAIRS_CF:
        for precision in T.precisions(loader, epi):
            K = 16 if (epi in (MAX, MAXCF) or loader in T.GATHERS) else 0
            pr = T.make(loader, epi, precision, 16, 24, B=2, n=3 if K else 40, K=K, C1=4 if loader == INTERP else 0)
            assert T.reference(pr).shape == (pr.out_rows, 24) and torch.isfinite(T.reference(pr, rounded=True)).all()


# ------------------------------------------------------------------------------------------------------ the restatement

def test_float64_restatement_equals_conv1d_grouping_and_interpolation():
    """product + epilogue against torch.nn.functional.conv1d (groups), amax over K, and the loaders against their
    definitions written the other way round (gather by loop, interpolation by index_select)."""
    import torch.nn.functional as F
    pr = T.make(PLAIN, STORE, F16X2, 20, 24, n=70, groups=3, relu=1)
    x = F.conv1d(pr.A.double().t().unsqueeze(0), pr.W.double().reshape(-1, 20, 1), pr.bias.double().reshape(-1), groups=3)
    assert float((T.reference(pr) - F.relu(x)[0].t()).abs().max()) < 1e-12
    pr = T.make(PLAIN, MAX, F16X2, 16, 24, n=5, K=16, relu=0)
    x = F.conv1d(pr.A.double().t().unsqueeze(0), pr.W.double().reshape(-1, 16, 1))[0].t()
    want = x.reshape(5, 16, 24).amax(dim=1) + pr.bias.double()
    assert float((T.reference(pr) - want).abs().max()) < 1e-12 and float(want.min()) < 0
    pr = T.make(PLAIN, MAXCF, F16X2, 16, 24, B=2, n=3, K=33)
    x = F.conv1d(pr.A.double().t().unsqueeze(0), pr.W.double().reshape(-1, 16, 1))[0].t()
    want = (x.reshape(6, 33, 24).amax(dim=1) + pr.bias.double()).clamp_min(0)
    assert float((T.reference(pr) - want).abs().max()) < 1e-12
    pr = T.make(GATHER, STORE, F16X2, 8, 24, B=2, n=3, K=16)
    a = T.rows(pr)
    for p in (0, 17, 48, 95):
        b, m, j = p // 48, p % 48 // 16, int(pr.gidx.reshape(-1)[p])
        want = torch.cat([pr.F[b * T.NPTS + j], pr.xyz[b, :, j] - pr.ctr[b, :, m]]).double()
        assert torch.equal(a[p], want), p
    pr = T.make(INTERP, STORE, F16X2, 8, 24, B=2, n=30, C1=4)
    a = T.rows(pr)
    for p in (0, 29, 30, 59):
        b = p // 30
        idx, w = pr.nidx.reshape(-1, 3)[p].long() + b * pr.N2, pr.nw.reshape(-1, 3)[p].double()
        want = torch.cat([(pr.S[idx].double() * w[:, None]).sum(0), pr.dense[p].double()])
        assert float((a[p] - want).abs().max()) < 1e-15, p
    pr = T.make(PLAIN, CF, F16X2, 16, 21, B=3, n=37, relu=0, heads=(3, 9, 4, 5), sigmoid_from=14)
    v = pr.A.double() @ pr.W[0].double().t() + pr.bias[0].double()
    want = torch.cat([v[:, :14], 1 / (1 + torch.exp(-v[:, 14:]))], dim=1)
    assert float((T.reference(pr) - want).abs().max()) < 1e-12


def test_rounded_yardstick_rounds_the_a_and_w_hi_planes_only():
    pr = T.make(PLAIN, STORE, BF16, 16, 24, n=33)
    bf = lambda x: x.to(torch.bfloat16).double()      # noqa: E731
    want = (bf(pr.A) @ bf(pr.W[0]).t() + pr.bias[0].double()).clamp_min(0)
    assert torch.equal(T.reference(pr, rounded=True), want) and not torch.equal(T.reference(pr), want)
    from s4g_release_amd.fused import split_bf16x3
    assert torch.equal(split_bf16x3(pr.W)[0].double(), bf(pr.W))          # the plane the kernel reads


def test_scale_is_tile_scale_per_column_tile_and_joins_the_tiles_of_a_group():
    pr = T.make(PLAIN, STORE, F16X2, 16, 40, B=3, n=65)
    ref = T.reference(pr)
    p = torch.arange(pr.P)
    want = CR.tile_scale(ref, p // 65, p // 128)[:, 0].expand(-1, 40)
    assert torch.equal(T.scale(pr, ref), want)
    wide = T.make(PLAIN, STORE, F16X2, 16, 260, n=5)             # two 128-column tiles and a 4-column one
    ref = torch.ones(5, 260, dtype=torch.float64)
    ref[:, 130] = 70.0
    s = T.scale(wide, ref)
    assert s[:, :128].eq(1).all() and s[:, 128:256].eq(70).all() and s[:, 256:].eq(1).all()
    grp = T.make(PLAIN, MAXCF, F16X2, 16, 8, B=2, n=1, K=200, scene_mags=(1.0, 1.0))     # rows 0..199 | 200..399
    ref = torch.ones(2, 8, dtype=torch.float64)
    ref[1] = 9.0
    assert T.scale(grp, ref).eq(9).all()                          # tile 1 (rows 128..255) holds rows of both groups


@pytest.mark.parametrize("zero", [False, True])
def test_guard_detects_a_stray_write_in_every_layout(zero):
    for kw in (dict(), dict(ldc=49), dict(c_coff=5, ldc=52), dict(shift=1), dict(groups=2, c_gcol=44), dict(c_coff=0)):
        def fresh():
            go = T.Guard("cpu", 5, 40, zero_payload=zero, **kw)
            go._owed(go.buf)[:] = 1.0
            return go
        go = fresh()
        go.check()
        assert not go.untouched() and T.Guard("cpu", 5, 40, zero_payload=zero, **kw).untouched()
        assert (go.out.data_ptr() % 16 == 0) == (kw.get("shift", 0) == 0)
        assert go.values().shape == (5, 40 * kw.get("groups", 1)) and go.values().eq(1).all()
        G0, n = go.GUARD, go.n
        inside = [G0 + go.c_coff + 40 * kw.get("groups", 1) + (4 if "c_gcol" in kw else 0), G0 + 2 * go.ldc + go.ldc - 1]
        if "c_gcol" in kw:
            inside.append(G0 + go.ldc + go.c_coff + 41)           # the gap between two groups' blocks
        if go.c_coff:
            inside.append(G0 + 3 * go.ldc + go.c_coff - 1)
        for word in [G0 - 1, G0 + n, 0, G0 + n + 255] + inside:
            go = fresh()
            go.buf[word] = 2.0
            with pytest.raises(AssertionError, match="written outside"):
                go.check()
        if not zero:
            go = fresh()
            go._owed(go.buf)[4, 0, 39] = float("nan")
            with pytest.raises(AssertionError, match="not finite"):
                go.check()


def test_outs_read_back_every_layout_as_the_matrix():
    """Channels-first tensors, the (B, Cout, M) max tensor and the two-output pair written the way the kernels index them
    come back as the (rows, Cout) matrix."""
    pr = T.make(PLAIN, CF, F16X2, 16, 21, B=3, n=5, relu=0, heads=(3, 9, 4, 5))
    outs, ref = T.Outs(pr, "cpu"), T.reference(pr).float()
    starts = [0, 3, 12, 16, 21]
    for h, g in enumerate(outs.g):
        ch = pr.heads[h]
        for row in range(pr.P):
            b, pt = divmod(row, 5)
            for cl in range(ch):
                g.out[(b * ch + cl) * 5 + pt] = ref[row, starts[h] + cl]
    outs.check()
    assert torch.equal(outs.matrix(), ref)
    pr = T.make(PLAIN, MAXCF, F16X2, 16, 7, B=2, n=3, K=5)
    outs, ref = T.Outs(pr, "cpu"), T.reference(pr).float()
    assert not outs.g[0].values().any()                           # zero-filled for the atomicMax merge
    for grp in range(6):
        b, m = divmod(grp, 3)
        for c in range(7):
            outs.g[0].out[(b * 7 + c) * 3 + m] = ref[grp, c]
    outs.check()
    assert torch.equal(outs.matrix(), ref)
    pr = T.make(PLAIN, STORE, F16X2, 16, 768, n=3, split_n=256)
    outs = T.Outs(pr, "cpu")
    f = outs.fields()
    assert f["c_coff"] == 0 and f["ldc"] % 4 == 0 and f["ldc2"] % 4 == 0 and f["ldc"] > 256 and f["ldc2"] > 512


# ------------------------------------------------------------------------------------- conditions on the GPU tests' inputs

def _argmax_rows(pr):
    """Per (group, channel) the row inside the group that holds the maximum, and the pre-activation maximum."""
    y = T.product(pr, T.rows(pr))
    y3 = y.view(-1, pr.K, y.shape[1])
    return y3.argmax(dim=1), y3.amax(dim=1) + pr.bias.double().reshape(1, -1)


def _max_families():
    fam = {}
    for loader, K, nc, relu in G.F_CASES:
        fam.setdefault(("f", loader, relu), []).append(G.case_f(loader, F16X2, K, nc, relu))
    for K in G.G_M:
        for B in (1, 3):
            for cout in (1, 72, 128, 129):
                fam.setdefault(("g", "cfirst" if cout == 72 else "plain", 1), []).append(G.case_g(F16X2, K, B, cout))
    for cf in (0, 4, 28, 32, 60):
        fam.setdefault(("i", GATHER, 1), []).append(G.case_i_gather(F16X2, cf, MAX))
    return fam


def test_max_families_place_maxima_at_the_edges_and_have_negative_groups():
    bm = T.geometry().GM_BM
    for key, cases in _max_families().items():
        first = last = before = after = neg = 0
        for pr in cases:
            arg, pre = _argmax_rows(pr)
            row = torch.arange(pr.out_rows)[:, None] * pr.K + arg            # the loader row of every maximum
            first += int((arg == 0).sum())
            last += int((arg == pr.K - 1).sum())
            before += int(((row % bm == bm - 1) & (row + 1 < pr.P)).sum())   # the last row in front of a tile boundary
            after += int(((row % bm == 0) & (row > 0)).sum())                # the first row behind one
            if key[2]:
                assert (pre < 0).any(), (key, pr.K, pr.n)                    # a ReLU case: a negative maximum
                neg += 1
            else:
                assert (T.reference_cached(pr) < 0).any(), (key, pr.K, pr.n)  # relu = 0: a negative result
        print(key, "first %d last %d before a tile boundary %d behind one %d" % (first, last, before, after))
        assert first and last and before and after, key
    g = _max_families()[("g", "plain", 1)]
    ends = {(b * pr.n + m + 1) * pr.K % bm for pr in g for b in range(pr.B) for m in range(pr.n)}
    assert 0 in ends and any(0 < e < 64 for e in ends) and any(e > 64 for e in ends)       # on, behind, in front of a tile end
    straddle = [pr for pr in g if pr.K > 1 and any((i * pr.K) // bm != ((i + 1) * pr.K - 1) // bm for i in range(pr.out_rows))]
    assert {pr.K for pr in straddle} >= {31, 33, 127, 129, 256, 300}
    for pr in straddle:                                   # in a straddling group: maxima on either side of the boundary
        arg, _ = _argmax_rows(pr)
        row = torch.arange(pr.out_rows)[:, None] * pr.K + arg
        t0 = (torch.arange(pr.out_rows)[:, None] * pr.K) // bm
        if pr.Cout > 1:
            assert (row // bm == t0).any() and (row // bm > t0).any(), (pr.K, pr.B, pr.Cout)


def test_straddling_scene_cases_have_scenes_2_to_the_10_apart_in_one_tile():
    bm = T.geometry().GM_BM
    for loader in (PLAIN, T.IADD):
        for rps in (64, 192):
            pr = G.case_j(loader, rps)
            p = torch.arange(pr.P)
            worst = 0.0
            for t in range(-(-pr.P // bm)):
                sc = (p[p // bm == t] // rps).unique().tolist()
                if len(sc) > 1:
                    m = [pr.scene_mags[s] for s in sc]
                    worst = max(worst, max(m) / min(m))
            assert worst >= 2.0 ** 10, (loader, rps, worst)
            assert pr.amax.shape == (pr.B, 64) and torch.equal(pr.amax.amax(dim=1), (pr.A if loader == PLAIN else pr.S)
                                                               .view(pr.B, -1).abs().amax(dim=1))
    assert (torch.arange(384) // 128).equal(torch.arange(384) // G.case_j(PLAIN, 128).rps)        # 128: a scene is a tile


# ------------------------------------------------------------------------------------------------- the fp32 bound

def _fp32_cases():
    for P in T.ROWS:
        yield G.case_a(FP32, P)
    for c in T.COLS:
        yield G.case_b(FP32, c)
    for cin in T.DEPTH8:
        yield G.case_c(FP32, cin)
    for cin in (1, 3, 5, 33):
        yield G.case_c_cf(FP32, cin)
    for g in (1, 2, 5):
        yield G.case_d(FP32, g)
    for loader, K, nc, relu in G.F_CASES:
        yield G.case_f(loader, FP32, K, nc, relu)
    for K in G.G_M:
        for B in (1, 3):
            for cout in (1, 72, 128, 129):
                yield G.case_g(FP32, K, B, cout)
    for loader in (PLAIN, CFIRST):
        for cf_N in (4, 36, 37, 128, 130):
            for heads, sig in G.H_HEADS:
                yield G.case_h(loader, FP32, cf_N, heads, sig)
    for cf in (0, 4, 28, 32, 60):
        for epi in (STORE, MAX):
            yield G.case_i_gather(FP32, cf, epi)
    for loader in (GIDX, REL4, GADD):
        yield G.case_i_family(loader, FP32)
    for c2, c1 in ((4, 0), (4, 12), (36, 0), (36, 12)):
        yield G.case_i_interp(FP32, c2, c1)
    for dense in (True, False):
        yield G.case_i_iadd(FP32, dense)
    yield G.case_i_cfirst(FP32)


def test_fp32_bound_is_four_times_the_cpu_fp32_products_own_distance():
    """The plain fp32 CPU product (torch) of every fp32 case of the GPU suite against float64 at the tile-and-scene
    scale: no case exceeds FP32_CPU_DISTANCE, the worst comes within a factor two of it, the bound is four times it."""
    worst, where = 0.0, None
    for pr in _fp32_cases():
        d = float(T.rel_err(T.fp32_cpu(pr), T.reference(pr), pr).max())
        if d > worst:
            worst, where = d, (pr.loader, pr.epi, pr.Cin, pr.Cout, pr.B, pr.n, pr.K)
    print("fp32 CPU product against float64: worst %.3e at %s; FP32_CPU_DISTANCE %.1e, bound %.1e"
          % (worst, where, T.FP32_CPU_DISTANCE, T.bounds(FP32)["max"]))
    assert T.FP32_CPU_DISTANCE / 2 <= worst <= T.FP32_CPU_DISTANCE
    assert T.bounds(FP32)["max"] == 4 * T.FP32_CPU_DISTANCE


# -------------------------------------------------------------------------------------------------------- sabotage table

def _ratio(pr, bad):
    """How far the sabotaged reference lies from the true one, in units of the bound the GPU case asserts."""
    return float(T.rel_err(bad, T.reference_cached(pr), pr).max()) / T.bounds(pr.precision)["max"]


def _sabotage_table():
    a = G.case_a(F16X2, 129)
    yield "1 row blocks swapped", _ratio(a, T.swap_row_blocks(T.reference_cached(a)))
    b = G.case_b(F16X2, 129)
    yield "2 last partial column tile dropped", _ratio(b, T.drop_last_partial_strip(T.reference_cached(b), T.col_tile(b)))
    yield "3 neighbouring block's bias", _ratio(b, T.reference(b, bias=T.neighbour_block_bias(b)))
    f = G.case_f(PLAIN, F16X2, 16, 9, 1)
    yield "4 group boundary a row late", _ratio(f, T.reference(f, group_shift=1))
    g = G.case_g(F16X2, 300, 3, 129)
    yield "5 straddling group keeps one side", _ratio(g, T.reference(g, one_side=True))
    c = G.case_c(F16X2, 48)
    assert c.Kpad16 % T.geometry().H2_BK == 16
    yield "6 half-deep last K step dropped", _ratio(c, T.reference(c, A=T.drop_half_step(c)))
    i = G.case_i_gather(F16X2, 28)
    yield "7a xyz columns dropped", _ratio(i, T.reference(i, A=T.rows(i, no_xyz=True)))
    yield "7b xyz columns a chunk off", _ratio(i, T.reference(i, A=T.rows(i, xyz_at=i.C - 4)))
    yield "8 scene of the tile's first row", _ratio(i, T.reference(i, A=T.rows(i, scene=T.first_row_scene(i))))
    n = G.case_i_interp(F16X2, 36, 12)
    yield "9 interpolation weights rotated", _ratio(n, T.reference(n, A=T.rows(n, nw=n.nw.roll(1, dims=2))))
    yield "10 dense columns dropped", _ratio(n, T.reference(n, A=T.rows(n, no_dense=True)))
    j = G.case_j(PLAIN, 192)
    yield "11 previous scene's scale", _ratio(j, T.reference(j, A=T.previous_scene_scale(j)))
    e = G.case_e_split(F16X2, T.WIDE_SPLIT[2] - 1)
    yield "12 out2 a tile off", _ratio(e, T.out2_off_by_a_tile(e, T.reference_cached(e)))
    h = G.case_h(PLAIN, F16X2, 37, (3, 9, 4, 5), 14)
    yield "13 point index not reduced", _ratio(h, T.cf_point_not_reduced(h, T.reference_cached(h)))
    yield "14 sigmoid a channel late", _ratio(h, T.reference(h, sigmoid_from=15))
    yield "15 head boundary a channel late", _ratio(h, T.head_boundary_off(h, T.reference_cached(h)))


def test_sabotaged_references_miss_the_gpu_bounds_by_a_margin():
    """One entry per wiring error, on the inputs of the GPU case named in the module's docstring."""
    table = list(_sabotage_table())
    for name, ratio in table:
        print("%-40s %12.0f x the bound" % (name, ratio))
    assert len(table) == 16 and len({n.split()[0].rstrip("ab") for n, _ in table}) == 15
    worst = min(table, key=lambda t: t[1])
    assert worst[1] >= BAR, worst
