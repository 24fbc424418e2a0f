"""The float64 yardstick of the local grasp search (tests/local_search_ref.py) against the fixture the reference's own
`finger_hand` produced (tests/golden/local_search.npz), `LocalSearchConfig` against the reference's constants, the C
ABI's declarations, and exact hand constructions.  No GPU."""
import os

import numpy as np

from tests import golden_util as GU
from tests import local_search_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
    from s4g_release_amd.postprocess import LocalSearchConfig
    return LocalSearchConfig(**kw)


def test_the_yardstick_reproduces_the_fixture():
    fx = GU.load("local_search.npz")
    cfg = _cfg()
    y = LR.search64(fx["points"], fx["frames"], fx["cloud"], fx["normals"], fx["labels"], cfg)
    assert LR.decided(y).all()
    assert np.array_equal(y["search_score"], fx["search_score"])
    assert np.array_equal(y["objects_label"], fx["objects_label"])
    assert np.array_equal(y["valid"], fx["valid"])
    assert np.abs(y["antipodal_score"] - fx["antipodal_score"]).max() <= 1e-4 + float(fx["margin"][0])
    vi = np.nonzero(fx["valid"])[0]
    assert len(vi) >= 8 and np.array_equal(y["valid_index"][:len(vi)], vi) and y["count"] == len(vi)
    assert np.abs(LR.frames_of(fx["points"], fx["frames"], cfg)[vi] - fx["valid_frame"][vi]).max() <= 1e-5
    for r, name in enumerate(LR.REASONS):                      # every outcome of a placement occurs
        assert (y["reason"] == r).any(), name
    assert (np.abs(fx["frames"]).sum((1, 2)) == 0).any()


def test_the_config_equals_the_references_constants():
    fx = GU.load("local_search.npz")
    c = _cfg()
    got = [c.table_height, c.num_points_threshold, c.back_collision_threshold, c.back_collision_margin,
           c.finger_collision_threshold, c.close_region_min_points, np.float32(c.neighbor_depth), c.half_bottom_width,
           c.bottom_length, c.finger_width, c.half_hand_thickness, c.finger_length, c.half_bottom_space,
           c.table_collision_offset, c.no_label]
    assert np.array_equal(np.array(got, np.float64), fx["constants"])
    assert c.no_label == 122 and c.shape == (4, 12)
    assert np.array_equal(np.array(c.length_search, np.float64), fx["length_search"])
    tb = c.tables()
    for k, f in (("depth", "depth_f32"), ("cos", "cos_f32"), ("sin", "sin_f32")):
        assert tb[k].dtype.is_floating_point and np.array_equal(tb[k].numpy(), fx[f]), k
    S = c.search_to_local().numpy()
    assert np.abs(S[..., :3, :3] @ np.swapaxes(S[..., :3, :3], -1, -2) - np.eye(3)).max() < 1e-6


def test_the_cabi_declares_both_entries_and_the_header_names_them():
    from s4g_release_amd import _cabi
    header = open(os.path.join(ROOT, "include", "s4g_ops.h")).read()
    for name, nargs in (("s4g_local_search_f32", 23), ("s4g_local_search_workspace_bytes", 5)):
        assert name in _cabi.SIGNATURES and len(_cabi.SIGNATURES[name][1]) == nargs
        assert name + "(" in header
    assert _cabi.S4G_ABI_VERSION == 14
    import s4g_release_amd
    assert callable(s4g_release_amd.grade_local_search)


def test_a_point_on_each_side_of_every_face():
    """Identity frame, roll 0: local coordinates are the cloud's.  The yardstick's counts are those of the strict
    inequalities written out by hand on the cloud itself."""
    cfg = LR.face_config()
    pts, frm, cloud, normals, labels = LR.face_scene(cfg)
    y = LR.search64(pts, frm, cloud, normals, labels, cfg, band_f32=True)
    k = LR.constants(cfg)
    x, yy, z = cloud.astype(np.float64)
    for d in range(2):
        slab = (x > k["lo"][d]) & (x < k["hi"][d])
        zin = (z < k["hht"]) & (z > -k["hht"])
        assert y["slab_count"][0, d] == slab.sum()
        assert y["back"][0, d, 0] == (slab & zin & (np.abs(yy) < k["hbw"]) & (x - k["depth"][d] < -k["m"])).sum()
        assert y["finger"][0, d, 0] == (slab & zin & (np.abs(yy) < k["hbw"]) & (np.abs(yy) > k["hbs"])).sum()
        close = slab & zin & (np.abs(yy) < k["hbs"])
        assert y["close"][0, d, 0] == close.sum() == y["search_score"][0, d, 0]
    f32 = np.float32
    on = lambda v, axis: int(((cloud[axis] == f32(v))).sum())
    assert on(k["hbs"], 1) == 1 and on(-k["hbs"], 1) == 1 and on(k["hht"], 2) == 1 and on(k["hbw"], 1) == 1
    # the three points at +half_bottom_space: on it and above it are finger / nothing, one ulp below is the extremum
    assert cloud[1].max() > k["hbw"] and (cloud[1] == f32(k["hbs"])).any()
    # bands: extremum Y, bound Y - 2^-8: strictly above the bound = the extremum, the point one ulp above the bound,
    # the points AT +-half_bottom_space are not in the close region
    Y = float(np.nextafter(f32(k["hbs"]), f32(-1)))
    cy = cloud[1][(np.abs(cloud[1]) < k["hbs"]) & (np.abs(cloud[2]) < k["hht"]) & (cloud[0] > k["lo"][1]) & (cloud[0] < k["hi"][1])]
    n_left = (cy > Y - 2.0 ** -8).sum()
    assert n_left == 3 and (cy < -(Y - 2.0 ** -8)).sum() == 3
    # each band: the extremum twice (|n.y| 0.125; one ulp inside half_bottom_space is in the cloud twice) and the point
    # one ulp past the bound (1.0): mean 1.25 / 3 on both sides; the point ON the bound (1.0) is not in the band
    assert abs(y["antipodal_score"][0, 1, 0] - (1.25 / 3) ** 2) < 1e-12


def test_eight_corners_straddling_the_table_offset():
    """A frame looking along +x at height h, roll 0 and 90 degrees (about): the lowest corners sit half_hand_thickness
    (roll 0) or half_bottom_width (roll 90) below the origin."""
    cfg = _cfg(theta_search_deg=(0, -90), length_search=(-0.02,), table_height=0.0, table_collision_offset=0.005)
    k = LR.constants(cfg)
    frm = np.eye(3, dtype=np.float32)[None]
    cloud = np.zeros((3, 1), np.float32)
    for h, want in ((0.005 + k["hht"] + 1e-4, [False, True]), (0.005 + k["hht"] - 1e-4, [True, True]),
                    (0.005 + k["hbw"] + 1e-4, [False, False]), (0.005 + k["hbw"] - 1e-4, [False, True])):
        y = LR.search64(np.array([[0, 0, h]], np.float32), frm, cloud, cloud, np.zeros(1, np.int32), cfg)
        assert y["gate"][0] and list(y["table_collision"][0, 0]) == want, h


def test_the_slab_threshold_is_strict():
    """num_points_threshold - 1 points in a slab skip its placements; exactly num_points_threshold do not."""
    cfg = LR.face_config(num_points_threshold=8, close_region_min_points=1, length_search=(-0.0625,))
    frm = np.eye(3, dtype=np.float32)[None]
    for n, reason in ((7, 2), (8, 0)):
        cloud = np.zeros((3, n), np.float32)
        cloud[0] = -0.015625
        cloud[1] = np.linspace(-0.01, 0.01, n)
        normals = np.tile(np.array([[0], [1], [0]], np.float32), (1, n))
        y = LR.search64(np.zeros((1, 3), np.float32), frm, cloud, normals, np.ones(n, np.int32), cfg)
        assert y["slab_count"][0, 0] == n and y["reason"][0, 0, 0] == reason
        assert y["search_score"][0, 0, 0] == (n if reason == 0 else 0) and bool(y["valid"][0]) == (reason == 0)
