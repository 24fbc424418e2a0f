"""The batched frame grading on the device (`postprocess.eval_frames`, csrc/eval_frames.hip; the reference's
`EvalExpCloud.eval_frame`, eval_experiment/eval_point_cloud.py:39-113) against the fixture the reference produced, the
float64 yardstick and the exact constructions of tests/eval_ref.py (checked on the CPU by tests/test_eval_ref.py).

Score tolerance: 1e-4 of float64 (the scale is 1).  Measured maxima: profiles/r09_eval_frames.md."""
import numpy as np
import pytest
import torch

from tests import collision_ref as CR
from tests import eval_ref as ER
from tests import golden_util as GU

pytestmark = pytest.mark.gpu

NAMES = ER.INT_FIELDS + ("collision",) + ER.FLOAT_FIELDS


def _run(dev, poses, cloud, normals, labels, gripper, inverse="general", count=None):
    from s4g_release_amd import postprocess as PP
    t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return PP.eval_frames(t(poses), t(cloud), t(normals), t(labels), gripper, inverse=inverse,
                          count=None if count is None else torch.as_tensor(count).to(dev))


def _np(r):
    out = {k: getattr(r, k).cpu().numpy() for k in NAMES}
    for k in ER.INT_FIELDS + ("collision",):
        out[k] = out[k].astype(np.int64)
    return out


def _same(a, b):
    return torch.equal(a.ints, b.ints) and torch.equal(a.floats.view(torch.int32), b.floats.view(torch.int32))


def _check_floats(got, want, where, what):
    """means and score within SCORE_TOL of float64 on the poses `where`; the extrema within fp32 rounding of them (1e-5:
    a local coordinate is a sum of three products of magnitude up to 3.4 -- the clearance scenes' pose grid -- and a
    translation, each rounded to an fp32 ulp of 2.4e-7 there)."""
    for k in ("mean_left", "mean_right", "score"):
        err = np.abs(got[k].astype(np.float64) - want[k])[where]
        print("%s: max |%s - float64| = %.3g over %d poses" % (what, k, err.max() if err.size else 0.0, err.size))
        assert (err <= ER.SCORE_TOL).all(), (what, k, err.max())
    for k in ("left_y", "right_y"):
        assert (np.abs(got[k].astype(np.float64) - want[k]) <= 1e-5).all(), (what, k)


def test_fixture_of_the_reference(dev):
    """On every decided pose the flags equal the reference's; back / finger / close within the pose's ambiguous counts of
    float64; scores within 1e-4 of float64 (and of the reference's, whose own distance is the stored margin)."""
    fx = GU.load("post_eval.npz")
    gripper = CR.gripper_config(False)
    y = ER.grade64(fx["g2l"], fx["cloud"], fx["normals"], fx["labels"], gripper)
    ok = ER.decided(y, gripper)
    got = _np(_run(dev, fx["poses"][None], fx["cloud"][None], fx["normals"][None], fx["labels"][None], gripper, "se3"))
    got = {k: v[0] for k, v in got.items()}
    assert np.array_equal(got["collision"][ok].astype(bool), fx["collision"][ok])
    assert np.array_equal(got["multi_objects"][ok].astype(bool), fx["multi_objects"][ok])
    assert np.array_equal((got["score"] != 0)[ok], (fx["antipodal_score"] != 0)[ok])
    for k, a in (("back", "amb_back"), ("finger", "amb_finger"), ("close", "amb_close")):
        assert (np.abs(got[k] - y[k]) <= y[a]).all(), k
    _check_floats(got, y, ok, "fixture")
    err = np.abs(got["score"].astype(np.float64) - fx["antipodal_score"])[ok]
    assert err.max() <= ER.SCORE_TOL + float(fx["margin"][0])
    scored = ok & (fx["antipodal_score"] != 0)
    assert np.array_equal(got["n_left"][scored], y["n_left"][scored])       # (no point near a band bound: generator)
    assert np.array_equal(got["n_right"][scored], y["n_right"][scored])
    # the same two integers as the collision counter, bit for bit
    from s4g_release_amd import postprocess as PP
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for inverse in ("se3", "general"):
        r = _run(dev, fx["poses"][None], fx["cloud"][None], fx["normals"][None], fx["labels"][None], gripper, inverse)
        _, counts = PP.view_non_collision(t(fx["poses"][None]), t(fx["cloud"][None]), gripper, inverse=inverse)
        assert torch.equal(r.ints[..., :2], counts), inverse


@pytest.mark.parametrize("B,N,K", ER.EDGE_SHAPES)
def test_clearance_scenes_at_the_loop_edges(dev, B, N, K):
    """All six integers exact (`==`) by construction, means and score against float64, back / finger equal to the
    collision counter's, for both inverses, with and without `count=` (padding rows read zero)."""
    from s4g_release_amd import postprocess as PP
    gripper, poses, cloud, normals, labels, exp = ER.edge_scene(B, N, K)
    d = [torch.from_numpy(a).to(dev) for a in (poses, cloud, normals, labels)]
    # the first scene's list ends just past a pass boundary of the pose loop (513 of 1 100: the second pass partly
    # live, the third never entered), or in the middle of the first pass
    cnt = np.array([513 if K > 513 else (K + 1) // 2, K, 0][:B])
    for inverse in ("general", "se3"):
        g2l = PP.se3_inverse(d[0]) if inverse == "se3" else torch.linalg.inv(d[0].double()).float()
        y = ER.grade64_batch(g2l, d[1], d[2], d[3], gripper)
        for count in (None, cnt):
            r = _run(dev, *d, gripper, inverse, count)
            got = _np(r)
            live = np.ones((B, K), bool) if count is None else np.arange(K)[None] < count[:, None]
            for k in ER.INT_FIELDS:
                assert np.array_equal(got[k][live], exp[k][live]), (inverse, count is None, k)
            assert np.array_equal(got["collision"][live].astype(bool), y["collision"][live])
            _check_floats({k: np.where(live, v, 0) for k, v in got.items()},
                          {k: np.where(live, v, 0) for k, v in y.items()}, live, "edge %s" % ((B, N, K),))
            for k in NAMES:
                assert (got[k][~live] == 0).all(), k
            _, counts = PP.view_non_collision(d[0], d[1], gripper, inverse=inverse,
                                              count=None if count is None else torch.as_tensor(count).to(dev))
            assert torch.equal(r.ints[..., :2], counts), inverse


@pytest.mark.parametrize("odd", [False, True])
def test_points_on_the_faces_and_band_bounds(dev, odd):
    """Signed-permutation poses: points exactly on, one ulp inside and one ulp outside each face of the close region and
    each band bound count exactly."""
    gripper = ER.face_gripper(odd)
    poses, cloud, normals, labels, exp = ER.face_scene(gripper)
    for inverse in ("general", "se3"):
        for count in (None, np.array([24])):
            got = _np(_run(dev, poses, cloud, normals, labels, gripper, inverse, count))
            for k in ER.INT_FIELDS + ("collision",):
                assert np.array_equal(got[k], exp[k].astype(np.int64)), (inverse, k)
            assert np.array_equal(got["left_y"].astype(np.float64), exp["left_y"])      # exact coordinates
            assert np.array_equal(got["right_y"].astype(np.float64), exp["right_y"])
            _check_floats(got, exp, np.ones_like(exp["scored"]), "faces")


def _natural(dev, B=3, N=40000, K=300, seed=4):
    """Fixture-like clouds for the behavioural tests: the fixture's scene, each scene of the batch a different
    subsample of it, with the fixture's poses repeated and jittered."""
    fx = GU.load("post_eval.npz")
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.permutation(fx["cloud"].shape[1])[:N] for _ in range(B)])
    cloud = np.stack([fx["cloud"][:, i] for i in idx])
    normals = np.stack([fx["normals"][:, i] for i in idx])
    labels = np.stack([fx["labels"][i] for i in idx])
    poses = fx["poses"][rng.integers(0, len(fx["poses"]), (B, K))].copy()
    poses[..., :3, 3] += rng.uniform(-0.002, 0.002, (B, K, 3)).astype(np.float32)
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (poses, cloud, normals, labels)]


def test_two_calls_are_bit_identical(dev):
    d = _natural(dev)
    a = _run(dev, *d, None, "se3")
    assert (a.score > 0).sum() > 20 and a.collision.any() and a.multi_objects.any()
    for _ in range(3):
        assert _same(a, _run(dev, *d, None, "se3"))


def test_a_scene_alone_equals_the_scene_in_its_batch(dev):
    d = _natural(dev)
    cnt = torch.tensor([300, 200, 17], device=dev)
    full = _run(dev, *d, None, "general", cnt)
    for b in range(3):
        one = _run(dev, *[t[b:b + 1].contiguous() for t in d], None, "general", cnt[b:b + 1])
        assert torch.equal(one.ints[0], full.ints[b]) and torch.equal(one.floats[0].view(torch.int32),
                                                                      full.floats[b].view(torch.int32)), b


def test_graph_capture_and_replay(dev):
    d = _natural(dev)
    cnt = torch.tensor([300, 250, 100], device=dev)
    eager = _run(dev, *d, None, "se3", cnt)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        _run(dev, *d, None, "se3", cnt)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _run(dev, *d, None, "se3", cnt)
    for _ in range(2):
        out.ints.zero_()
        out.floats.zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        assert _same(out, eager)


def test_a_scene_with_nan_coordinates_is_contained(dev):
    """One scene of the batch holds NaN and inf coordinates: the call returns and the clean scenes' outputs are
    bit-identical to a run without that scene (its own outputs are unspecified)."""
    d = _natural(dev)
    clean = _run(dev, *[t[[0, 2]].contiguous() for t in d], None, "se3")
    d[1][1, 0, 77::5] = float("nan")
    d[1][1, 2, 1000] = float("inf")
    d[2][1, 1, 50:60] = float("nan")
    bad = _run(dev, *d, None, "se3")
    torch.cuda.synchronize(dev)
    for i, b in enumerate((0, 2)):
        assert torch.equal(bad.ints[b], clean.ints[i])
        assert torch.equal(bad.floats[b].view(torch.int32), clean.floats[i].view(torch.int32))


def test_refuses_cpu_tensors_and_wrong_shapes(dev):
    from s4g_release_amd import postprocess as PP
    d = _natural(dev, B=1, N=1000, K=4)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        PP.eval_frames(d[0], d[1].cpu(), d[2], d[3])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        PP.eval_frames(d[0], d[1], d[2], d[3].cpu())
    with pytest.raises(RuntimeError, match="int32"):
        PP.eval_frames(d[0], d[1], d[2], d[3].long())
    with pytest.raises(RuntimeError, match="scene_normals"):
        PP.eval_frames(d[0], d[1], d[2][:, :, :999].contiguous(), d[3])
    with pytest.raises(RuntimeError, match="float32"):
        PP.eval_frames(d[0], d[1].double(), d[2], d[3])
    with pytest.raises(ValueError):
        PP.eval_frames(d[0], d[1], d[2], d[3], inverse="other")


def test_detector_evaluate_equals_eval_frames_by_hand(dev):
    from s4g_release_amd import postprocess as PP
    from s4g_release_amd.detector import GraspDetector
    from tests.test_detector_gpu import _clouds
    net = GU.shipped_net(dev)
    det = GraspDetector(net, topk=2048, seed=1)
    cloud = _clouds(30000, [2, 3])
    d = torch.from_numpy(cloud).to(dev)
    out = det.detect_device(d, num_selected=5, score_threshold=0.6, verticalness_threshold=-2.0)
    rng = np.random.default_rng(3)
    normals = torch.from_numpy(np.stack([ER.noisy_normals(rng, 30000) for _ in range(2)])).to(dev)
    labels = torch.from_numpy(rng.integers(0, 3, (2, 30000)).astype(np.int32)).to(dev)
    cand, sel = det.evaluate(out, d, normals, labels)
    H, _, _, count = out.candidates
    by_hand = PP.eval_frames(H, d, normals, labels, det.gripper, inverse="se3", count=count)
    assert _same(cand, by_hand)
    assert _same(sel, PP.eval_frames(out[0], d, normals, labels, det.gripper, inverse="se3", count=out[2]))
    assert int(count.min()) > 5 and int((cand.close > 0).sum()) > 0
    # the selected poses are candidates: each one's grade is among its scene's candidate grades
    for b in range(2):
        rows = {tuple(r.tolist()) for r in cand.ints[b, :int(count[b])]}
        assert all(tuple(r.tolist()) in rows for r in sel.ints[b, :int(out[2][b])])
