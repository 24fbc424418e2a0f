"""CPU tests of the float64 yardstick of the baseline inputs (tests/close_region_ref.py) against the reference's own
outputs (tests/golden/baseline_regions.npz, tools/gen_golden_baseline.py), of the constants, of the C ABI's names, of
hand constructions whose answer is known exactly, and of deliberate mistakes the yardstick must notice."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from s4g_release_amd.postprocess import LocalSearchConfig, ProjectionConfig
from tests import close_region_ref as CR
from tests import local_search_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG, PROJ = LocalSearchConfig(), ProjectionConfig()


@pytest.fixture(scope="module")
def fx():
    return CR.load_fixture()


@pytest.fixture(scope="module")
def y64(fx):
    """The yardstick's run of the whole fixture, computed once: best placement, matrices, regions and maps."""
    L, T = CFG.shape
    F = len(fx["points"])
    s = LR.search64(fx["points"], fx["frames"], fx["cloud"], fx["normals"], np.zeros(fx["cloud"].shape[1], np.int32), CFG)
    s64 = s["antipodal_score"].reshape(F, L * T)
    return dict(scores=s64, **_pipeline(fx, s64))


def _pipeline(fx, s64, best=None, region=None, projection=None):
    bi, bs, bv = CR.best64(s64, best)
    G = CR.g2l64(fx["points"], fx["frames"], CFG, bi)
    reg = CR.regions64(G, fx["cloud"], CFG, sabotage=region)
    maps, sets = [], []
    for f in np.nonzero(fx["valid"])[0]:
        r = reg[f]
        idx = np.sort(np.concatenate([r["certain"], r["ambiguous"]])) if r["local"] is not None else np.zeros(0, np.int64)
        if region == "face_ge" or len(r["ambiguous"]) == 0:
            idx = r["certain"]
        p32 = r["local"][:, idx].astype(np.float32) if len(idx) else np.zeros((3, 0), np.float32)
        n32 = (G[f][:3, :3] @ fx["normals"][:, idx].astype(np.float64)).astype(np.float32)
        maps.append(CR.projection64(p32, n32, PROJ, CFG, projection)[0])
        sets.append((idx, p32, n32))
    return dict(index=bi, score=bs, valid=bv, g2l=G, regions=reg, maps=np.stack(maps), sets=sets)


def test_fixture_holds_its_cases(fx):
    v = fx["valid"]
    assert v.sum() >= 20 and (~v).sum() >= 1 and float(fx["margin"][0]) < 1e-6
    assert len(fx["set_offset"]) == v.sum() + 1 and fx["set_offset"][-1] == len(fx["set_index"])
    assert fx["maps"].shape == (v.sum(), 12, 60, 60) and (fx["maps"] != 0).mean() < 0.1


def test_yardstick_reproduces_the_reference(fx, y64):
    assert np.array_equal(y64["valid"], fx["valid"]) and np.array_equal(y64["index"], fx["best_index"])
    assert np.abs(y64["score"] - fx["score"]).max() <= 1e-5
    vf = np.nonzero(fx["valid"])[0]
    assert np.abs(y64["g2l"][vf] - fx["baseline_frame"][vf]).max() <= 1e-5
    n_clear, worst, seen, total = 0, 0.0, 0, 0
    for k, f in enumerate(vf):
        r = y64["regions"][f]
        ref_idx = fx["set_index"][fx["set_offset"][k]:fx["set_offset"][k + 1]]
        assert set(r["certain"]) <= set(ref_idx) <= set(r["certain"]) | set(r["ambiguous"])
        if len(r["ambiguous"]):
            continue
        n_clear += 1
        assert np.array_equal(r["certain"], ref_idx)
        idx, p32, n32 = y64["sets"][k]
        mask = CR.pixel_mask(r["local"][:, idx], PROJ, CFG)
        bound = CR.map_bound(p32, n32, PROJ, CFG) + float(fx["margin"][0])
        d = np.abs(y64["maps"][k] - fx["maps"][k])
        assert (d <= bound)[~mask].all(), (f, float((d * ~mask).max()))
        worst = max(worst, float((d * ~mask).max()))
        nz = fx["maps"][k] != 0
        seen, total = seen + int((nz & ~mask).sum()), total + int(nz.sum())
    print("largest distance from the reference's maps %.3g on %d frames, %d of %d non-zero pixels compared"
          % (worst, n_clear, seen, total))
    assert n_clear >= 0.75 * len(vf) and seen >= 0.9 * total


def test_constants_equal_the_references(fx):
    c = fx["constants"]
    assert (CFG.finger_length, CFG.bottom_length, CFG.half_bottom_space, CFG.half_hand_thickness) == tuple(c[:4])
    assert PROJ.dims(CFG) == tuple(c[7:10])
    assert (PROJ.resolution, PROJ.margin) == tuple(int(v) for v in fx["resolution"])
    assert PROJ.units(CFG) == tuple(float(np.float32(v)) for v in c[4:7])
    h = CR.heights64(PROJ, CFG)
    for a in range(3):                                  # torch.linspace(unit / 2, dim - unit / 2, R)
        assert abs(h[a][0] - 0.5 * c[4 + a]) < 1e-15 and abs(h[a][-1] - (c[7 + a] - 0.5 * c[4 + a])) < 1e-12
        h0, hs = PROJ.heights(CFG)[a]
        assert np.abs(h0 + hs * np.arange(60) - h[a]).max() < 60 * 2.0 ** -24 * c[7 + a]
    with pytest.raises(ValueError):
        ProjectionConfig(resolution=65).check()


def _declared(text, name):
    return re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S)) is not None


def test_header_and_cabi_name_the_entries():
    from s4g_release_amd import _cabi
    header = open(os.path.join(ROOT, "include", "s4g_ops.h")).read()
    abi = header[header.index(" * 14:"):header.index("#define S4G_ABI_VERSION")]
    for name, nargs in (("s4g_best_placement_f32", 14), ("s4g_close_region_workspace_bytes", 4),
                        ("s4g_close_region_f32", 21)):
        assert name in abi and _declared(header, name) and len(_cabi.SIGNATURES[name][1]) == nargs, name
    assert _cabi.S4G_ABI_VERSION == 14 and "#define S4G_ABI_VERSION 14" in header
    import s4g_release_amd as pkg
    assert callable(pkg.best_placement) and callable(pkg.close_regions) and callable(pkg.label_baseline_view)


@pytest.mark.parametrize("x_range", [None, (0.0, CFG.finger_length)])
def test_faces_are_strict(x_range):
    cloud, member = CR.face_cloud(CFG, x_range)
    r = CR.regions64(np.eye(4)[None], cloud, CFG, x_range, tol=0.0)[0]
    assert np.array_equal(r["certain"], np.nonzero(member)[0]) and len(r["ambiguous"]) == 0
    wrong = CR.regions64(np.eye(4)[None], cloud, CFG, x_range, tol=0.0, sabotage="face_ge")[0]
    assert len(wrong["certain"]) == member.sum() + 2        # the two points exactly on the y faces
    near = CR.regions64(np.eye(4)[None], cloud, CFG, x_range)[0]
    assert len(near["ambiguous"]) == 18 and np.array_equal(near["certain"], [0])


def test_voxel_rule_at_the_faces():
    u = CR.units32(PROJ, CFG)
    for a in range(3):
        for k in (1, 7, 30, 59, 60):
            for c in CR._ulps(np.float32(k) * u[a]):
                q = Fraction(float(np.float32(c))) / Fraction(float(u[a]))
                want = int(np.floor(np.float32(float(q))))          # the correctly rounded fp32 quotient, then floor
                p = np.zeros((3, 1), np.float32)
                p[a] = c
                got, ok = CR.voxels32(p, PROJ, CFG)
                assert got[a, 0] == want and bool(ok[0]) == (want < 60)
    assert not CR.voxels32(np.array([[-1e-9], [0], [0]], np.float32), PROJ, CFG)[1][0]


def test_opposite_normals_and_a_line_of_two():
    u = CR.units32(PROJ, CFG).astype(np.float64)
    H = CR.heights64(PROJ, CFG)
    centre = lambda v: [(v[a] + 0.5) * u[a] for a in range(3)]
    pts = np.array([centre((3, 4, 5)), centre((3, 4, 5)), centre((3, 4, 9)), centre((3, 4, 9))], np.float32).T
    nrm = np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32).T
    m, most = CR.projection64(pts, nrm, PROJ, CFG)
    assert most == 2 and np.count_nonzero(m[0]) == 1
    assert m[0, 3, 4] == (H[2][5] + H[2][9]) / 2                    # two occupied voxels on the z line of pixel (3, 4)
    assert tuple(m[1:4, 3, 4]) == (0.25, 0.0, 0.25)                 # (mean 0 + mean (0.5, 0, 0.5)) / 2
    assert m[4, 4, 5] == H[0][3] and tuple(m[5:8, 4, 5]) == (0, 0, 0)    # mean 0 with occupancy 1
    assert m[8, 9, 3] == H[1][4] and tuple(m[9:12, 9, 3]) == (0.5, 0, 0.5)


@pytest.mark.parametrize("stage,name", [("best", "later_on_tie"), ("region", "no_y_shift"), ("projection", "voxel_sum"),
                                        ("projection", "order"), ("projection", "height_axis"),
                                        ("projection", "occ_count"), ("projection", "div_points")])
def test_sabotage_is_noticed(fx, y64, stage, name):
    """Each mistake moves at least 20 map pixels or at least 3 frames' verdicts on the fixture.  (`>=` instead of `>` on
    a face cannot: no point of a random scene lies exactly on one.  test_faces_are_strict holds it to the points built
    on the faces.)"""
    bad = _pipeline(fx, y64["scores"], **{stage: name})
    frames = int((bad["index"] != y64["index"]).sum())
    pixels = int((np.abs(bad["maps"] - y64["maps"]) > 1e-6).sum())
    print(name, frames, "frames,", pixels, "pixels")
    assert frames >= 3 or pixels >= 20
