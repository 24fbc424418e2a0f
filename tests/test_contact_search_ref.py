"""CPU checks of the contact model's label path: the float64 yardstick of tests/contact_search_ref.py against the
fixture the reference's own `run_score` produced (tests/golden/contact_search.npz, tools/gen_golden_contact_search.py),
the C ABI's three new entries, `ContactSearchConfig`, and the proof that the fixture sees every mistake of
`contact_search_ref.SABOTAGES`."""
import os
import re

import numpy as np
import pytest

from tests import contact_search_ref as CR
from tests import golden_util as GU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return GU.load("contact_search.npz")


@pytest.fixture(scope="module")
def yard(fx):
    return CR.label(fx["reference_cloud"], fx["cloud"], fx["scene"], fx["scene_normals"], fx["labels"], fx["camera"],
                    fx["g2l"], fx["frame_point_index"], fx["search_score"], fx["antipodal_score"],
                    float(fx["radius"][0]), frame_count=int(fx["frame_count"][0]))


def test_fixture_holds_what_it_is_for(fx, yard):
    g, nn, s = yard
    n = int(fx["frame_count"][0])
    kf, kp = CR.decided(g, nn, s, fx["frame_point_index"])
    assert np.array_equal(kf, fx["keep_frames"]) and np.array_equal(kp, fx["keep_points"])
    assert (~kf).sum() <= 0.02 * len(kf) and (~kp).sum() <= 0.02 * len(kp)
    fm, fail = kf[:n], g["fail"][:n]
    assert (g["valid"][:n][fm] == 1).sum() >= 40
    for bit in (CR.FAIL_TABLE, CR.FAIL_FINGER, CR.FAIL_BEHIND, CR.FAIL_LABELS):
        assert ((fail & bit) != 0)[fm].sum() >= 20, bit
    assert not (fail & (CR.FAIL_EMPTY | CR.FAIL_NONFINITE)).any() or not g["raises"][:n].any()
    assert (np.bincount(fx["frame_point_index"][:n]) >= 2).sum() >= 30
    e = np.exp(6.5)
    assert (fx["search_score"][:n] >= e).any() and (fx["search_score"][:n] < e).any()
    assert (nn[0] < 0).sum() >= 12
    assert (g["valid"][n:] == 0).all() and (g["fail"][n:] == 0).all() and (g["label"][n:] == CR.Config.no_label).all()


def test_yardstick_against_the_reference(fx, yard):
    g, nn, s = yard
    n = int(fx["frame_count"][0])
    kf, kp = fx["keep_frames"], fx["keep_points"]
    graded = (fx["ref_frame_valid"] >= 0) & kf
    assert graded[:n].sum() > 0.5 * n and not graded[n:].any()
    assert np.array_equal(fx["ref_frame_valid"][graded], g["valid"][graded])
    assert np.array_equal(fx["ref_frame_label"][graded], g["label"][graded])
    rvi, yvi = fx["ref_valid_index"], s["valid_index"][:s["count"]]
    kept = yvi[kp[yvi]]
    assert np.array_equal(rvi[kp[rvi]], kept) and len(kept) >= 100
    pos = {int(v): k for k, v in enumerate(rvi)}
    rows = np.array([pos[int(v)] for v in kept])
    bf = s["best_frame"][kept]
    assert np.array_equal(fx["ref_search_score"][rows], fx["search_score"][bf])
    assert np.array_equal(fx["ref_antipodal_score"][rows], fx["antipodal_score"][bf])
    assert np.array_equal(fx["ref_objects_label"][rows], g["label"][bf])
    inv64 = np.linalg.inv(fx["g2l"].astype(np.float64))
    want = np.linalg.inv(fx["camera_pose"]) @ inv64[bf]
    assert np.abs(fx["ref_valid_frame"][rows] - want).max() <= float(fx["inverse_distance"][0]) + 4e-7
    assert np.abs(CR.rigid_inverse(fx["g2l"]) - inv64).max() < 1e-6           # rigid inputs: the two inverses agree
    assert np.nanmax(np.abs(fx["ref_normals"] - s["normals"])[kp]) < 1e-12


def test_fp32_restatement_and_margin(fx, yard):
    g, nn, s = yard
    y32 = CR.label(fx["reference_cloud"], fx["cloud"], fx["scene"], fx["scene_normals"], fx["labels"], fx["camera"],
                   fx["g2l"], fx["frame_point_index"], fx["search_score"], fx["antipodal_score"],
                   float(fx["radius"][0]), frame_count=int(fx["frame_count"][0]), dtype=np.float32)
    kf, kp = fx["keep_frames"], fx["keep_points"]
    for k in ("ints", "table", "valid", "label", "fail"):
        assert np.array_equal(y32[0][k][kf], g[k][kf]), k
    assert np.array_equal(y32[2]["best_frame"][kp], s["best_frame"][kp])
    d = np.abs(y32[2]["point_score"].astype(np.float64) - s["point_score"])[kp].max()
    assert d == float(fx["margin"][0]) and 0 < d < 2.5e-7               # a few ulp of scores of size at most 1


def test_empty_close_region_is_bit_4(fx):
    assert fx["empty_raised"].all() and len(fx["empty_raised"]) >= 20
    g = CR.grade(fx["empty_g2l"], fx["scene"], fx["labels"])
    assert g["raises"].all() and (g["valid"] == 0).all() and ((g["fail"] & CR.FAIL_EMPTY) != 0).all()
    assert (g["label"] == CR.Config.no_label).all()


def _declared(text, name):
    return re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S)) is not None


def test_header_and_cabi_name_the_entries():
    from s4g_release_amd import _cabi
    header = open(os.path.join(ROOT, "include", "s4g_ops.h")).read()
    abi = header[header.index(" * 14:"):header.index("#define S4G_ABI_VERSION")]
    for name in ("s4g_contact_search_f32", "s4g_match_nearest_f32", "s4g_contact_select_f32"):
        assert name in abi and _declared(header, name) and name in _cabi.SIGNATURES, name
    assert _cabi.S4G_ABI_VERSION == 14 and "#define S4G_ABI_VERSION 14" in header
    src = open(os.path.join(ROOT, "s4g_release_amd", "csrc", "contact_search.hip")).read()
    for n, word in enumerate(("empty close region", "rigid inverse", "not finite", "centred box"), 1):
        assert "(%d)" % n in src and word in src and word in header, word


def test_config_limits_and_bounds_rounded_once():
    import torch
    from s4g_release_amd import postprocess as PP
    cfg, ref = PP.ContactSearchConfig(), CR.Config()
    for k in ("width_search", "height_search", "length_search", "table_height", "table_collision_offset",
              "back_collision_margin", "half_bottom_width", "bottom_length", "finger_width", "half_hand_thickness",
              "finger_length", "no_label", "half_bottom_space"):
        assert getattr(cfg, k) == getattr(ref, k), k
    assert cfg.shape == (3, 3, 1) and cfg.placements == 9 and PP.CS_MAX_LIST == 4
    assert (PP.FAIL_TABLE, PP.FAIL_FINGER, PP.FAIL_BEHIND, PP.FAIL_LABELS, PP.FAIL_EMPTY, PP.FAIL_NONFINITE) == \
        (CR.FAIL_TABLE, CR.FAIL_FINGER, CR.FAIL_BEHIND, CR.FAIL_LABELS, CR.FAIL_EMPTY, CR.FAIL_NONFINITE)
    PP.ContactSearchConfig(width_search=(0,) * 4, height_search=(0,) * 4, length_search=(0,) * 4).check()
    for k in ("width_search", "height_search", "length_search"):
        for bad in ((), (0,) * 5):
            with pytest.raises(ValueError):
                PP.ContactSearchConfig(**{k: bad}).check()
    tb = cfg.tables()
    hht, hbs = ref.half_hand_thickness, ref.half_bottom_space
    want = {"zlo": [-hht + d for d in ref.height_search], "zhi": [hht + d for d in ref.height_search],
            "ylo": [-hbs + d for d in ref.width_search], "yhi": [hbs + d for d in ref.width_search],
            "dy": list(ref.width_search), "xlo": [-ref.bottom_length + d for d in ref.length_search],
            "xhi": [ref.finger_length + d for d in ref.length_search]}
    for k, v in want.items():
        assert tb[k].dtype == torch.float32
        assert np.array_equal(tb[k].numpy(), np.array(v, np.float64).astype(np.float32)), k
    # one rounding is not two: the sum of the rounded parts differs from the rounded sum on some bound
    twice = [np.float32(np.float32(hbs) + np.float32(d)) for d in ref.width_search] + \
            [np.float32(np.float32(-hbs) + np.float32(d)) for d in ref.width_search] + \
            [np.float32(np.float32(s * hht) + np.float32(d)) for d in ref.height_search for s in (1, -1)]
    once = [np.float32(hbs + d) for d in ref.width_search] + [np.float32(-hbs + d) for d in ref.width_search] + \
           [np.float32(s * hht + d) for d in ref.height_search for s in (1, -1)]
    assert any(a != b for a, b in zip(twice, once))
    # torch compares an fp32 tensor with a Python scalar in fp32: the bound as a Python float, then one rounding
    b = hbs + 0.005
    x = torch.tensor([np.float32(b)])
    assert not bool((x < b).any()) and bool((x.double() < b).any()) == (float(np.float32(b)) < b)


def test_the_table_check_sees_the_centred_box_only():
    """A frame whose centred box clears the table limit by 2 mm: a box shifted 5 mm down would not.  The reference's
    nine search matrices alias one identity, so this is NOT a table collision."""
    cfg = CR.Config()
    limit = cfg.table_height + cfg.table_collision_offset
    g = np.eye(4, dtype=np.float32)[None].copy()
    g[0, 2, 3] = -(limit + cfg.half_hand_thickness + 0.002)             # horizontal frame, origin 14 mm above the limit
    scene = np.array([[0.02], [0.0], [limit + cfg.half_hand_thickness + 0.002]], np.float32)
    out = CR.grade(g, scene, np.array([7], np.int32), cfg)
    assert out["table"][0] == 0 and out["fail"][0] == 0 and out["valid"][0] == 1 and out["label"][0] == 7
    bad = CR.grade(g, scene, np.array([7], np.int32), cfg, sabotage=("real_table",))
    assert bad["table"][0] == 1 and bad["valid"][0] == 0
    g[0, 2, 3] += 0.003                                                 # 1 mm below: the centred box collides
    assert CR.grade(g, scene, np.array([7], np.int32), cfg)["table"][0] == 1


@pytest.mark.parametrize("name", CR.SABOTAGES)
def test_the_fixture_sees_the_mistake(fx, yard, name):
    n = CR.altered_rows(fx, name, base=yard)
    print("%s alters %d kept rows" % (name, n))
    assert n >= 10, (name, n)


def test_later_frame_wins_a_tie_and_nan_propagates():
    one = np.ones(3, np.float32)
    kw = dict(nearest_idx=np.array([0]), cloud=np.zeros((3, 1), np.float32),
              scene_normals=np.array([[0], [0], [2.0]], np.float32), camera=np.array([0, 0, 1], np.float32),
              frame_point_index=np.zeros(3, np.int32), valid=np.ones(3, np.int32))
    s = CR.select(search=100 * one, antipodal=0.5 * one, **kw)
    assert s["best_frame"][0] == 2 and s["count"] == 1 and np.array_equal(s["normals"][0], [0, 0, 1])
    assert CR.select(search=100 * one, antipodal=0.5 * one, sabotage=("earlier_wins",), **kw)["best_frame"][0] == 0
    s = CR.select(search=np.array([100, -1, 50], np.float32), antipodal=0.5 * one, **kw)      # log(-1) = NaN in the middle
    assert s["best_frame"][0] == 2 and abs(s["point_score"][0] - np.log(50.0) / 6.5 * 0.5) < 1e-7
    s = CR.select(search=np.array([100, 50, -1], np.float32), antipodal=0.5 * one, **kw)      # ... and last: the score is NaN
    assert s["best_frame"][0] == -1 and np.isnan(s["point_score"][0]) and s["count"] == 0


def test_the_gpu_edge_ladder_follows_the_kernel_constants():
    """tests/test_contact_search_gpu.py places its shapes around the kernel's sweep, chunk and frame-pass sizes: they are
    read out of csrc/contact_search.hip here, so a moved constant fails this test until the ladder follows."""
    src = open(os.path.join(ROOT, "s4g_release_amd", "csrc", "contact_search.hip")).read()
    c = {k: int(v) for k, v in re.findall(r"constexpr int (CS_[A-Z_]+) = (\d+);", src)}
    gpu = open(os.path.join(ROOT, "tests", "test_contact_search_gpu.py")).read()
    m = re.search(r"SWEEP, CHUNK, MIN_CHUNKS, MAX_CHUNKS = (\d+), (\d+), (\d+), (\d+)", gpu)
    assert tuple(map(int, m.groups())) == (256 * c["CS_U"], c["CS_CHUNK_POINTS"], c["CS_MIN_CHUNKS"], c["CS_MAX_CHUNKS"])
    m = re.search(r"WG_PASS, SCENE_PASS = (\d+), (\d+)", gpu)
    assert tuple(map(int, m.groups())) == (c["CS_SLOTS"], c["CS_SLOTS"] * c["CS_GX"])
    assert c["CS_MAX_LIST"] == 4 and "WG_PASS * 64" in gpu and c["CS_GX"] == 64
