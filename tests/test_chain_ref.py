"""CPU checks of what tests/test_chain_edges_gpu.py stands on (tests/chain_ref.py): the float64 restatement against an
independent formulation, the guarded buffer's own detection, and the sabotage table -- on the GPU tests' OWN inputs,
each wiring error the chain kernel's structure makes possible must move the reference by >= 100 x the bound the GPU case
asserts (the bar tests/test_heads_ref.py set), so a kernel with that error cannot pass.

Measured ratios (miss / bound, the miss relative to the row's tile scale; inf: the sabotaged value is not finite):

    1  two 32-row blocks of a wave swapped           f16x2 a C=128 pair P=129              20 000 x
    2  two 64-channel wave slices swapped            f16x2 a C=128 pair P=129              33 000 x
    3  the last partial strip dropped                f16x2 c C=128 Cout=192 STORE          33 000 x
    4  a strip read with the previous strip's bias   f16x2 c C=128 Cout=256 STORE          23 000 x
    5  group g read with group g+1's weights         f16x2 d C=256 groups=2                32 000 x
    6  second K-chunk of a deep first layer dropped  f16x2 a C=256 deep512 P=65             9 800 x
    7  max over 32 instead of 64 rows                f16x2 b plain C=128 nc=3               9 600 x
    8  a centroid's max merged into its neighbour    bf16  b plain C=128 nc=3                 130 x
    9  a scene scaled by the previous scene's max    f16x2 e plain C=128 (B, N) = (3, 65)       inf
    10 relu2 applied where it is off                 f16x2 f pair STORE C=128 relus=(1, 0)  33 000 x
    11 the xyz term of GATHER_ADD dropped            f16x2 b gadd C=128 nc=9                2 400 x

(33 000 x = 1 / 3e-5: the miss is as large as the tile's scale itself.  Entry 9 is modelled as the plane split with the
wrong power of two, tests/chain_ref.f16x2_planes: a 40 x scene under a unit scene's scale overflows fp16's high plane and
the reference stops being finite; the opposite direction only costs the low plane's last bits and is NOT visible at
these bounds -- the upper pin on out_amax in family (e) is what holds a too-large scale.  Entry 8 is the smallest: the
bf16 bound is 2e-3 and neighbouring centroids' maxima differ by a quarter of the scale.)

The figures are printed by the test; the table is rounded down to two digits."""
import pytest
import torch

from tests import chain_ref as R
from tests.chain_ref import BF16, F16X2, GADD, MAX, PLAIN, STORE, STRIP, TILE

BAR = 100.0


def test_float64_restatement_equals_grouped_conv1d_and_amax():
    """chain() against torch.nn.functional.conv1d with groups, then amax over K: to 1e-12."""
    import torch.nn.functional as F
    for groups, C, K1, widths, relus, K in [(1, 128, 128, [192], (1, 1), 0), (5, 64, 128, [64], (1, 0), 0),
                                            (2, 64, 64, [64, 128], (0, 1, 1), 64), (1, 128, 256, [128, 64], (1, 1, 0), 64)]:
        g = torch.Generator(device="cpu").manual_seed(groups + C)
        P = 3 * 64
        A = torch.randn(P, groups * K1, generator=g, dtype=torch.float64)
        ins, outs = [K1] + [C] * len(widths), [C] + widths
        Ws = [torch.randn(groups, o, i, generator=g, dtype=torch.float64) for o, i in zip(outs, ins)]
        bs = [torch.randn(groups, o, generator=g, dtype=torch.float64) for o in outs]
        got = R.chain(A, Ws, bs, relus, groups, R.f64, K)
        x = A.t().unsqueeze(0)                                       # (1, groups K1, P)
        for W, b, relu in zip(Ws, bs, relus):
            x = F.conv1d(x, W.reshape(-1, W.shape[2], 1), b.reshape(-1), groups=groups)
            if relu:
                x = F.relu(x)
        want = x[0].t()
        if K:
            want = want.reshape(P // K, K, -1).amax(dim=1)
        assert got.shape == want.shape
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_bf16_yardstick_rounds_inputs_weights_and_hidden_activations():
    pr = R.problem(PLAIN, BF16, 128, (128,), STORE, 1, 33)
    bf = lambda x: x.to(torch.bfloat16).double()      # noqa: E731
    h = (bf(pr.A) @ bf(pr.Ws[0][0]).t() + pr.bs[0][0].double()).clamp_min(0)
    want = (bf(h.float()) @ bf(pr.Ws[1][0]).t() + pr.bs[1][0].double()).clamp_min(0)
    assert torch.equal(R.reference(pr, rounded=True), want)
    assert not torch.equal(R.reference(pr, rounded=False), want)


@pytest.mark.parametrize("zero", [False, True])
def test_guarded_buffer_detects_a_stray_write(zero):
    rows, cout, groups = 5, 64, 2

    def fresh():
        go = R.GuardedOut("cpu", rows, cout, groups, zero_payload=zero)
        go.values()[:] = 1.0
        return go

    go = fresh()
    assert go.ldc == cout * groups + 8 and go.c_coff == 4 and go.GUARD >= 256
    go.check()
    assert not go.untouched() and R.GuardedOut("cpu", rows, cout, groups, zero).untouched()
    G, n = go.GUARD, rows * go.ldc
    for word in (G - 1, G + n, G + 3, G + go.ldc - 4, G + 2 * go.ldc + go.c_coff - 1, 0, 2 * G + n - 1):
        go = fresh()
        go.buf[word] = 2.0                                          # one float before / behind / in a gap column
        with pytest.raises(AssertionError, match="written outside"):
            go.check()
    go = fresh()
    go.values()[3, 70] = float("nan")                               # an owed element left (or made) non-finite
    with pytest.raises(AssertionError, match="not finite"):
        go.check()
    if not zero:
        go = R.GuardedOut("cpu", rows, cout, groups)
        go.values()[:rows - 1] = 1.0                                # an owed row never written: the sentinel is a NaN
        with pytest.raises(AssertionError, match="not finite"):
            go.check()
        go.check(rows_owed=rows - 1)


def _ratio(pr, bad, name="max"):
    """How far the sabotaged reference lies from the true one, in units of the bound the GPU case asserts."""
    ref = R.reference_cached(pr, pr.precision == BF16)
    bd = R.bounds(pr.precision, 1 + len(pr.widths), pr.K1 > pr.C, pr.loader not in (PLAIN, R.IADD))[name]
    return float(R.rel_err(bad, ref, pr).max()) / bd


def _sabotage_table():
    a = R.problem(PLAIN, F16X2, 128, (128,), STORE, 1, 129)
    yield "1 row blocks swapped", _ratio(a, R.swap_row_blocks(R.reference_cached(a, False)))
    yield "2 wave slices swapped", _ratio(a, R.swap_wave_slices(R.reference_cached(a, False), STRIP[128]))
    c = R.problem(PLAIN, F16X2, 128, (192,), STORE, 1, TILE[(F16X2, 128)] + 1)
    yield "3 last partial strip dropped", _ratio(c, R.drop_last_partial_strip(R.reference_cached(c, False), STRIP[128]))
    c = R.problem(PLAIN, F16X2, 128, (256,), STORE, 1, TILE[(F16X2, 128)] + 1)
    yield "4 previous strip's bias", _ratio(c, R.reference(c, final_bias=R.previous_strip_bias(c, STRIP[128])))
    d = R.problem(PLAIN, F16X2, 256, (256,), STORE, 1, TILE[(F16X2, 256)] + 1, groups=2)
    yield "5 next group's weights", _ratio(d, R.reference(d, group_shift=1))
    deep = R.problem(PLAIN, F16X2, 256, (256,), STORE, 1, 65, K1=512)
    A = deep.A.double().clone()
    A[:, 256:] = 0.0
    yield "6 second K-chunk dropped", _ratio(deep, R.reference(deep, A=A))
    b = R.problem(PLAIN, F16X2, 128, (128,), MAX, 1, 3)
    yield "7 max over 32 rows", _ratio(b, R.reference(b, k_rows=32))
    b = R.problem(PLAIN, BF16, 128, (128,), MAX, 1, 3)
    yield "8 merged into the neighbour", _ratio(b, R.merge_into_neighbour(R.reference_cached(b, True)))
    e = R.problem(PLAIN, F16X2, 128, (128,), STORE, 3, 65)
    yield "9 previous scene's scale", _ratio(e, R.reference(e, A=R.previous_scene_scale(e)))
    f = R.problem(PLAIN, F16X2, 128, (128,), STORE, 1, TILE[(F16X2, 128)] + 1, relus=(1, 0))
    yield "10 relu2 where it is off", _ratio(f, R.reference(f, relus=(1, 1)))
    ga = R.problem(GADD, F16X2, 128, (128,), MAX, 3, 3)
    yield "11 xyz term dropped", _ratio(ga, R.reference(ga, no_xyz=True))


def test_sabotaged_references_miss_the_gpu_bounds_by_a_margin():
    """One entry per wiring error, on the inputs of the GPU case named in the module's docstring."""
    table = list(_sabotage_table())
    for name, ratio in table:
        print("%-32s %12.0f x the bound" % (name, ratio))
    assert len(table) == 11
    worst = min(table, key=lambda t: t[1])
    assert worst[1] >= BAR, worst


def test_scene_scale_model_overflows_and_keeps_the_right_scale_exact():
    """The plane-split model behind entry 9: with a row's own maximum the two fp16 planes carry 22 bits; with a bound far
    below it the high plane overflows."""
    x = torch.tensor([[3.0, -1.25e-3, 0.7]])
    ok = R.f16x2_planes(x, torch.tensor([3.0]))
    assert float((ok - x.double()).abs().max()) < 2.0 ** -20 * 3.0
    assert not torch.isfinite(R.f16x2_planes(x * 1000, torch.tensor([3.0]))).all()


def test_tile_scale_joins_the_scenes_of_a_tile_only():
    """A quiet scene is measured at its own scale unless a louder scene shares its tile."""
    ref = torch.ones(256, 4, dtype=torch.float64)
    ref[128:192] = 50.0                                            # scene 2 of four 64-row scenes
    scene = torch.arange(256) // 64
    s = R.tile_scale(ref, scene, torch.arange(256) // 128)[:, 0, 0]
    assert s[:128].eq(1.0).all() and s[128:].eq(50.0).all()
    s = R.tile_scale(ref, scene, torch.arange(256) // 64)[:, 0, 0]
    assert s[192:].eq(1.0).all() and s[128:192].eq(50.0).all()


def test_distinct_row_layouts_cover_the_boundaries_they_claim():
    for precision in (F16X2, BF16):
        pr = R.seg_problem(precision, 128, 256, 512)
        own = pr.owner[:256]
        for edge in (32, 64, 128, 192):                             # half-wave, wave, tile(s)
            assert own[edge - 1] == own[edge] and own[edge] >= 0
        assert (own[100:108] == -1).all() and (own[232:256] == -1).all()          # filler: in the run, at its end
        assert pr.seg_rows.tolist() == [256, 512, 0, 256]
        assert torch.isnan(pr.rel4[256:512]).all() and torch.isnan(pr.rel4[1024:1536]).all()
        assert torch.isfinite(pr.rel4[:256]).all() and torch.isfinite(pr.rel4[512:1024]).all()
        assert pr.seg4.shape[0] == pr.P // 4 and (pr.seg4[64:128] == -1).all()
        ref = R.seg_reference(pr)
        assert torch.isfinite(ref).all() and not ref[6:8].any() and not ref[16:24].any() and ref[:6].any()
        assert ref[8:16].amax() > 0
        full = R.chain(R.loader_rows(pr)[512:1024], pr.Ws, pr.bs, pr.relus, 1, R.f64, 64)
        assert torch.equal(ref[8:16], full)                        # the plain-layout scene is the 64-row form
