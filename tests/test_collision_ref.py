"""The exact collision references of tests/collision_ref.py checked on the CPU, before any GPU run: on both
constructions the oracle's restatement of the reference's `view_non_collision` (oracle/postprocess.py) returns exactly
the counts the construction promises, under both inverses the device offers, and the float64 classifier agrees with
zero ambiguous points where the construction keeps a clearance."""
import numpy as np
import pytest

from tests import collision_ref as CR

@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("inverse", ["general", "se3"])
@pytest.mark.parametrize("B,N,K", [(1, 1, 1), (3, 7, 17), (2, 3000, 40), (1, 9000, 150)])
def test_clearance_scene_counts_hold_by_construction(B, N, K, inverse, odd):
    gripper = CR.gripper_config(odd)
    poses, cloud, expected = CR.clearance_scene(np.random.default_rng(N + K), B, N, K, gripper)
    assert poses.dtype == cloud.dtype == np.float32 and cloud.shape == (B, 3, N)
    ok, counts = CR.oracle_counts(poses, cloud, gripper, inverse)
    assert np.array_equal(counts, expected)
    assert np.array_equal(ok, CR.verdicts(expected, gripper))
    c64, amb = CR.classify64(CR.global2local(poses, inverse), cloud, gripper, tol=1e-5)
    assert np.array_equal(c64, expected) and (amb == 0).all()
    if K >= 40:      # verdicts on both sides of both thresholds
        assert 0.2 < ok.mean() < 0.8
        assert (expected[..., 0] > 28).any() and (expected[..., 0] <= 28).any()
        assert (expected[..., 1] > 10).any() and (expected[..., 1] <= 10).any()


def test_clearance_scene_fills_a_large_cloud():
    gripper = CR.gripper_config(True)
    poses, cloud, expected = CR.clearance_scene(np.random.default_rng(0), 1, 20000, 3, gripper)
    ok, counts = CR.oracle_counts(poses, cloud, gripper, "se3")
    assert np.array_equal(counts, expected) and expected[0, 0].min() > 500        # pose 0's boxes take the fill
    c64, amb = CR.classify64(CR.global2local(poses, "general"), cloud, gripper, tol=1e-5)
    assert np.array_equal(c64, expected) and (amb == 0).all()


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("inverse", ["general", "se3"])
def test_face_scene_on_face_points_are_not_counted(inverse, odd):
    gripper = CR.gripper_config(odd)
    poses, cloud, expected = CR.face_scene(gripper)
    assert poses.shape == (1, 24, 4, 4)
    ok, counts = CR.oracle_counts(poses, cloud, gripper, inverse)
    assert np.array_equal(counts, expected)
    assert np.array_equal(ok, CR.verdicts(expected, gripper))
    # the inverses are exact transposes; the local coordinates are exact fp32 values
    g2l = CR.global2local(poses, inverse)
    assert np.array_equal(g2l[..., :3, :3], np.swapaxes(poses[..., :3, :3], -1, -2)) and (g2l[..., :3, 3] == 0).all()
    c64, amb = CR.classify64(g2l, cloud, gripper)
    assert np.array_equal(c64, expected) and amb.min() > 0
    assert len(set(map(tuple, expected[0]))) > 4          # counts differ from pose to pose


def test_face_scene_pins_strictness_and_the_margin():
    """The construction tells `<` from `<=` on every face, and a flipped margin: for fp32 coordinates `v <= f` is
    `v < nextafter(f, +inf)`, so moving one face by one ulp outward is the non-strict comparison -- it changes the
    counts of some pose, for the counter(s) that face decides."""
    gripper = CR.gripper_config(True)
    poses, cloud, expected = CR.face_scene(gripper)
    fc = CR.faces(gripper)
    loc = np.einsum("kji,jn->kin", poses[0, :, :3, :3].astype(np.float64), cloud[0].astype(np.float64))
    x, y, z = loc[:, 0], loc[:, 1], loc[:, 2]
    f32 = np.float32
    for face, out, decides in (("fl", np.inf, (1,)), ("bl", np.inf, (0, 1)), ("hht", np.inf, (0, 1)),
                               ("hbw", np.inf, (0, 1)), ("hbs", -np.inf, (1,)), ("m", -np.inf, (0,))):
        mut = dict(fc, **{face: float(np.nextafter(f32(fc[face]), f32(out)))})
        back, fing = CR._counts_local(x, y, z, mut)
        got = np.stack([back.sum(1), fing.sum(1)], 1)
        for c in decides:
            assert (got[:, c] != expected[0, :, c]).any(), (face, c)
    back, fing = CR._counts_local(x, y, z, dict(fc, m=-fc["m"]))
    assert (back.sum(1) != expected[0, :, 0]).all()


@pytest.mark.parametrize("B,N,K", CR.EDGE_SHAPES)
def test_edge_scenes_load_every_pass(B, N, K):
    """The exact GPU cases (tests/test_collision_gpu.py) pin every pass of the kernel's pose loop with points of its
    own, not only with zeros: from N = 8 on, every scene's last pose (in the last, partial pass) has points in its
    boxes; from N = 1 000 on, so has some pose of every pass, and where K > 1 024 the third pass has verdicts on both
    sides at the largest N."""
    gripper, poses, cloud, expected = CR.edge_scene(B, N, K)
    nz = expected.sum(-1) > 0
    if N >= 8:
        assert nz[:, K - 1].all()
    if N >= 1000:
        for p0 in range(0, K, CR.POSES_PER_PASS):
            assert nz[:, p0:p0 + CR.POSES_PER_PASS].any(axis=1).all(), p0
    if N >= 40000 and K > 2 * CR.POSES_PER_PASS:
        ok = CR.verdicts(expected, gripper)[:, 2 * CR.POSES_PER_PASS:]
        assert ok.any(axis=1).all() and (~ok).any(axis=1).all()
