"""The batched collision counter (`postprocess.view_non_collision`, csrc/pose_decode.hip `collision_counts_kernel`)
pinned EXACTLY at the shapes its loop structure turns on: 8 point chunks per scene (empty chunks below N = 50), sweeps
of 1 024 points, 16 workgroups sharing a scene's poses, 32 poses per pass (second pass from pose 512, third from
1 024).  The expected counts come from tests/collision_ref.py (clouds with a clearance from every face, points exactly
on the faces under exact transforms; the constructions themselves are checked on the CPU by
tests/test_collision_ref.py)."""
import numpy as np
import pytest
import torch

from tests import collision_ref as CR

pytestmark = pytest.mark.gpu

VARIANTS = [(inverse, with_count) for inverse in ("general", "se3") for with_count in (False, True)]


def _run(dev, poses, cloud, gripper, inverse, count=None):
    from s4g_release_amd import postprocess as PP
    ok, counts = PP.view_non_collision(torch.from_numpy(poses).to(dev), torch.from_numpy(cloud).to(dev), gripper,
                                       inverse=inverse, count=None if count is None else torch.as_tensor(count).to(dev))
    return ok.cpu().numpy(), counts.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("B,N,K", CR.EDGE_SHAPES)
def test_counts_are_exact_at_the_loop_edges(dev, B, N, K):
    gripper, poses, cloud, expected = CR.edge_scene(B, N, K)     # (every pass loaded: tests/test_collision_ref.py)
    want_ok = CR.verdicts(expected, gripper)
    for inverse, with_count in VARIANTS:
        ok, counts = _run(dev, poses, cloud, gripper, inverse, np.full(B, K) if with_count else None)
        assert np.array_equal(counts, expected), (inverse, with_count, np.argwhere(counts != expected)[:5])
        assert np.array_equal(ok, want_ok), (inverse, with_count)


@pytest.mark.parametrize("N,K", [(43, 513), (8193, 1100)])
def test_padded_pose_lists(dev, N, K):
    """`count=`: rows below clamp(count, 0, K) equal the unpadded call, the rest read zero counts and ok = False."""
    gripper = CR.gripper_config(odd=True)
    cnt = np.array([0, 1, 17, K, K + 5, -3])
    poses, cloud, expected = CR.clearance_scene(np.random.default_rng(K), len(cnt), N, K, gripper)
    for inverse in ("general", "se3"):
        ok_all, counts_all = _run(dev, poses, cloud, gripper, inverse)
        assert np.array_equal(counts_all, expected)
        ok, counts = _run(dev, poses, cloud, gripper, inverse, cnt)
        for b, c in enumerate(np.clip(cnt, 0, K)):
            assert np.array_equal(counts[b, :c], counts_all[b, :c]) and np.array_equal(ok[b, :c], ok_all[b, :c]), b
            assert (counts[b, c:] == 0).all() and not ok[b, c:].any(), b


@pytest.mark.parametrize("odd", [False, True])
def test_points_on_the_faces(dev, odd):
    """Points exactly on each decisive face (not counted) and one ulp either side, under exact transforms: the device
    counts equal the oracle's fp32 restatement and the construction's exactly."""
    gripper = CR.gripper_config(odd)
    poses, cloud, expected = CR.face_scene(gripper)
    for inverse in ("general", "se3"):
        rok, rcounts = CR.oracle_counts(poses, cloud, gripper, inverse)
        for with_count in (False, True):
            ok, counts = _run(dev, poses, cloud, gripper, inverse, np.array([24]) if with_count else None)
            assert np.array_equal(counts, expected) and np.array_equal(counts, rcounts), (inverse, with_count)
            assert np.array_equal(ok, rok)


def test_natural_clouds_against_float64(dev):
    """Tabletop scenes and decoded poses (K = 1 100: three passes): per pose and counter the device count is within
    the ambiguous points (closer than 4e-6 to a deciding face) of the float64 count, and the verdicts agree wherever
    that margin does not straddle the threshold."""
    from s4g_release_amd import postprocess as PP, synth
    rng = np.random.default_rng(21)
    B, N, K = 3, 25600, 1100
    pts = synth.make_batch([8, 9, 10], N)
    pred = {"score": rng.standard_normal((B, 3, N)).astype(np.float32),
            "frame_R": rng.standard_normal((B, 9, N)).astype(np.float32),
            "frame_t": rng.standard_normal((B, 4, N)).astype(np.float32)}
    d_pts = torch.from_numpy(pts).to(dev)
    H, _, _ = PP.decode_top_poses({k: torch.from_numpy(v).to(dev) for k, v in pred.items()}, d_pts, K)
    for odd in (False, True):
        gripper = CR.gripper_config(odd)
        for inverse in ("general", "se3"):
            g2l = PP.se3_inverse(H) if inverse == "se3" else torch.linalg.inv(H.double()).float()
            c64, amb = CR.classify64(g2l, d_pts, gripper, tol=4e-6)
            ok, counts = PP.view_non_collision(H, d_pts, gripper, inverse=inverse)
            counts = counts.cpu().numpy().astype(np.int64)
            assert (np.abs(counts - c64) <= amb).all(), (odd, inverse)
            thr = np.array([gripper.back_collision_threshold, gripper.finger_collision_threshold])
            settled = ((c64 - amb <= thr) == (c64 + amb <= thr)).all(axis=-1)
            assert settled.mean() > 0.9
            assert np.array_equal(ok.cpu().numpy()[settled], CR.verdicts(c64, gripper)[settled]), (odd, inverse)
            assert (c64 > 0).any()                        # the gripper does touch the table-top clouds
