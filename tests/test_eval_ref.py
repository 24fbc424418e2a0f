"""CPU tests of the grading yardstick (tests/eval_ref.py) and of the fixture the reference's own
`EvalExpCloud.eval_frame` produced (tests/golden/post_eval.npz, tools/gen_golden_eval.py): the yardstick reproduces the
reference, three deliberately wrong yardsticks do not, the constructions hold what they promise, and the library
carries the two new symbols."""
import ctypes

import numpy as np
import pytest

from tests import collision_ref as CR
from tests import eval_ref as ER
from tests import golden_util as GU


@pytest.fixture(scope="module")
def fx():
    return GU.load("post_eval.npz")


@pytest.fixture(scope="module")
def graded(fx):
    return ER.grade64(fx["g2l"], fx["cloud"], fx["normals"], fx["labels"], CR.gripper_config(False))


def _classes(fx):
    return ER.outcome(fx["collision"], fx["multi_objects"], fx["antipodal_score"] != 0)


def test_library_and_ctypes_table_carry_the_eval_symbols():
    from s4g_release_amd import _cabi
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in ("s4g_eval_frames_f32", "s4g_eval_frames_workspace_bytes"):
        assert name in _cabi.SIGNATURES, name
        assert hasattr(L, name), name
    f = _cabi.lib().s4g_eval_frames_workspace_bytes
    assert f(0, 100, 4) == 0 and f(2, 100, 4) > 0
    assert f(1, 409601, 50) > f(1, 200000, 50) > f(1, 1000, 50)       # more chunks for a larger cloud
    assert _cabi.lib().s4g_abi_version() == 14                          # an addition under 14


def test_fixture_holds_every_outcome(fx):
    cls = _classes(fx)
    assert 90 <= len(cls) <= 110 and fx["cloud"].shape[1] >= 40000
    for c in range(5):
        assert (cls == c).sum() >= 8, c
    assert set(np.unique(fx["labels"])) == set(range(13))
    n = np.linalg.norm(fx["normals"].astype(np.float64), axis=0)
    assert np.abs(n - 1).max() < 0.02 and np.abs(n - 1).max() > 1e-3    # noisy unit normals


def test_reference_flags_equal_the_yardstick_on_decided_poses(fx, graded):
    gripper = CR.gripper_config(False)
    ok = ER.decided(graded, gripper)
    cls = _classes(fx)
    for c in range(5):
        assert (~ok[cls == c]).sum() <= 0.1 * (cls == c).sum(), c         # at most 10 % undecided per class
    assert np.array_equal(fx["collision"][ok], graded["collision"][ok])
    assert np.array_equal(fx["multi_objects"][ok], graded["multi_objects"][ok])
    assert np.array_equal((fx["antipodal_score"] != 0)[ok], (graded["score"] != 0)[ok])


def test_reference_scores_lie_within_the_stored_margin(fx, graded):
    margin = float(fx["margin"][0])
    assert margin < 1e-5
    err = np.abs(fx["antipodal_score"].astype(np.float64) - graded["score"])
    assert err.max() <= margin, err.max()
    scored = fx["antipodal_score"] != 0
    assert scored.sum() >= 8 and fx["antipodal_score"][scored].std() > 0.01    # the scores carry signal


@pytest.mark.parametrize("sabotage", ["normals", "band_x"])
def test_a_wrong_yardstick_misses_the_fixture(fx, sabotage):
    """The normals left unrotated, or x in place of y in the band test: off by at least 100 times the score tolerance
    on at least half of the scored poses."""
    bad = ER.grade64(fx["g2l"], fx["cloud"], fx["normals"], fx["labels"], CR.gripper_config(False), sabotage=sabotage)
    scored = fx["antipodal_score"] != 0
    err = np.abs(bad["score"][scored] - fx["antipodal_score"][scored])
    assert (err >= 100 * ER.SCORE_TOL).mean() >= 0.5, np.sort(err)[::-1][:5]


def _exactly_fifty():
    """One pose (the identity) over a scene with exactly 50 close-region points of one label, no collision."""
    rng = np.random.default_rng(5)
    gripper = CR.gripper_config(False)
    fc = ER.params(gripper)
    n = 50
    pts = np.stack([rng.uniform(0.01, fc["fl"] - 0.01, n), rng.uniform(-fc["hbs"] + 0.002, fc["hbs"] - 0.002, n),
                    rng.uniform(-fc["hht"] + 0.001, fc["hht"] - 0.001, n)]).astype(np.float32)
    far = rng.uniform(0.5, 1.0, (3, 200)).astype(np.float32)
    cloud = np.concatenate([pts, far], 1)
    labels = np.concatenate([np.full(n, 4), rng.integers(1, 9, 200)]).astype(np.int32)
    return np.eye(4, dtype=np.float32)[None], cloud, ER.noisy_normals(rng, cloud.shape[1]), labels, gripper


def test_min_points_gate_is_strict():
    """`close < 50` returns early (eval_point_cloud.py:107): a pose with exactly 50 close-region points IS scored; a
    yardstick gating with <= misses it."""
    g2l, cloud, normals, labels, gripper = _exactly_fifty()
    good = ER.grade64(g2l, cloud, normals, labels, gripper)
    assert good["close"][0] == 50 and good["scored"][0] and good["score"][0] > 0
    assert not good["collision"][0] and not good["multi_objects"][0]
    bad = ER.grade64(g2l, cloud, normals, labels, gripper, sabotage="min_points_ge")
    assert not bad["scored"][0] and bad["score"][0] == 0
    assert abs(bad["score"][0] - good["score"][0]) >= 100 * ER.SCORE_TOL


@pytest.mark.parametrize("B,N,K", [(1, 8193, 512), (3, 48902, 1100), (1, 1025, 511), (2, 7, 33)])
def test_clearance_scene_holds_by_construction(B, N, K):
    """The float64 classification of a clearance scene equals the constructed integers, no point is ambiguous, every
    pass of the kernel's pose loop holds points, and (where N allows) both sides of every gate occur."""
    gripper, poses, cloud, normals, labels, exp = ER.edge_scene(B, N, K)
    g2l = CR.global2local(poses, "general")
    r = ER.grade64_batch(g2l, cloud, normals, labels, gripper, tol=5e-5)
    for k in ER.INT_FIELDS:
        assert np.array_equal(r[k], exp[k]), k
    for k in ("amb_back", "amb_finger", "amb_close", "amb_left", "amb_right"):
        assert (r[k] == 0).all(), k
    if N >= 8000:
        assert (exp["close"][:, [j for j in (0, 511, 512, 1023, 1024, K - 1) if j < K]] > 0).all()
        assert {49, 50, 51} <= set(exp["close"].ravel())
        assert r["scored"].sum() >= 8 and r["collision"].any() and r["multi_objects"].any()
        sc = r["scored"]
        assert (exp["n_left"][sc] > 1).any() and (exp["n_right"][sc] > 1).any()
        span = (r["left_y"] - r["right_y"])[sc]
        assert (span / 3 < 0.005).any() and (span / 3 > 0.005).any()      # both branches of the depth's min


@pytest.mark.parametrize("odd", [False, True])
def test_face_scene_is_exact_and_scored(odd):
    gripper = ER.face_gripper(odd)
    poses, cloud, normals, labels, exp = ER.face_scene(gripper)
    assert exp["scored"].sum() >= 6                                      # poses whose bands are exercised
    # every coordinate under every pose is a coordinate of the cloud: exact
    Rs = poses[0, :, :3, :3].astype(np.float64)
    loc = np.einsum("kji,jn->kin", Rs, cloud[0].astype(np.float64))
    assert np.array_equal(loc, loc.astype(np.float32).astype(np.float64))
    # points exactly on a band bound exist for scored poses (and do not count: strict)
    bound = exp["left_y"][0] - 2.0 ** -8
    closer = (np.abs(loc[:, 2]) < ER.params(gripper)["hht"]) & (loc[:, 0] > 0) & (loc[:, 0] < ER.params(gripper)["fl"])
    on = (closer & (np.abs(loc[:, 1]) == bound[:, None])).sum(1)
    assert (on[exp["scored"][0]] > 0).sum() >= 6
    assert (exp["n_left"][0] != exp["n_right"][0]).any() and not exp["collision"].any()
