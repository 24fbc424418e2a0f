"""GPU parity of the device-side pose decode (next row f1) against the CPU
restatement of the reference's demo post-processing."""
import numpy as np
import pytest
import torch

from tests import collision_ref as CR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("convention", ["demo", "detector"])
def test_decode_top_poses_matches_oracle(dev, convention):
    from oracle import postprocess as OP
    from s4g_release_amd import postprocess as PP, synth
    rng = np.random.default_rng(5)
    B, N, K = 3, 4000, 50
    pts = synth.make_batch([1, 2, 3], N)
    pred = {"score": rng.standard_normal((B, 3, N)).astype(np.float32) * 2,
            "frame_R": rng.standard_normal((B, 9, N)).astype(np.float32),
            "frame_t": rng.standard_normal((B, 4, N)).astype(np.float32),
            "movable_logits": rng.random((B, 5, N)).astype(np.float32)}
    H, s, idx = PP.decode_top_poses({k: torch.from_numpy(v).to(dev) for k, v in pred.items()},
                                    torch.from_numpy(pts).to(dev), K, convention)
    rH, rs, ridx = OP.decode_top_poses(pred, pts, K, convention)
    assert tuple(H.shape) == (B, K, 4, 4)
    assert np.allclose(s.cpu().numpy(), rs, atol=2e-6)
    # same selection (scores are distinct for random logits), best first
    assert np.array_equal(idx.cpu().numpy(), ridx)
    assert np.allclose(H.cpu().numpy(), rH, atol=2e-5)
    Hn = H.cpu().numpy().astype(np.float64)
    RtR = np.einsum("bkij,bkil->bkjl", Hn[..., :3, :3], Hn[..., :3, :3])
    assert np.allclose(RtR, np.eye(3), atol=1e-5)                        # orthonormal frames
    assert np.allclose(np.linalg.det(Hn[..., :3, :3]), 1.0, atol=1e-5)   # right-handed


def test_expected_score_full_size(dev):
    from s4g_release_amd import postprocess as PP
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(2, 3, 25600, generator=g).to(dev)
    got = PP.expected_score(logits, "detector")
    ref = (torch.softmax(logits.double(), dim=1) *
           torch.tensor([1 / 3, 2 / 3, 1.0], dtype=torch.float64, device=dev)[None, :, None]).sum(1)
    assert (got.double() - ref).abs().max().item() < 1e-6


def test_batched_collision_check_matches_oracle(dev):
    """Row f2: counts of points behind the palm / inside the finger volumes for all
    poses in one launch vs the per-pose restatement of the reference."""
    from oracle import postprocess as OP
    from s4g_release_amd import postprocess as PP, synth
    rng = np.random.default_rng(9)
    B, N, K = 2, 25600, 40
    pts = synth.make_batch([4, 5], N)
    pred = {"score": rng.standard_normal((B, 3, N)).astype(np.float32),
            "frame_R": rng.standard_normal((B, 9, N)).astype(np.float32),
            "frame_t": rng.standard_normal((B, 4, N)).astype(np.float32)}
    H, _, _ = PP.decode_top_poses({k: torch.from_numpy(v).to(dev) for k, v in pred.items()},
                                  torch.from_numpy(pts).to(dev), K)
    ok, counts = PP.view_non_collision(H, torch.from_numpy(pts).to(dev))
    rok, rcounts = OP.view_non_collision(H.cpu().numpy(), pts)
    counts_np, ok_np = counts.cpu().numpy().astype(np.int64), ok.cpu().numpy()
    # Every disagreement must be explained by points that sit within a few fp32 ulps of a box
    # face (the 4x4 . 4xN product is summed in a different order on the two sides): classify the
    # points in float64 and count, per pose and per counter, those closer than `tol` to any face
    # that decides the counter -- the two counts may differ by at most that many.
    amb = CR.classify64(np.linalg.inv(H.cpu().numpy().astype(np.float64)).astype(np.float32), pts,
                        PP.GripperConfig(), tol=4e-6)[1]
    diff = np.abs(counts_np - rcounts)
    assert (diff <= amb).all(), np.argwhere(diff > amb)[:5]
    # verdicts differ only when a count sits at its threshold, give or take the ambiguous points
    at_edge = (np.abs(rcounts[..., 0] - 10 * np.sqrt(8)) <= amb[..., 0] + 1) | \
              (np.abs(rcounts[..., 1] - 10) <= amb[..., 1] + 1)
    assert (at_edge | (ok_np == rok)).all(), np.argwhere(~at_edge & (ok_np != rok))[:5]
    assert (ok_np == rok).mean() >= 0.95
    assert counts.cpu().numpy().sum() > 0          # the gripper does touch the table-top cloud


def test_detector_post_processing_matches_oracle(dev):
    """Row f1 as `GraspDetector.post_processing` defines it (grasp_detector.py:137-185): score
    threshold, descending order among survivors, verticalness filter with the caller's 3x3,
    translation decode + Gram-Schmidt, result in the caller's frame, variable-length per scene."""
    from oracle import postprocess as OP
    from s4g_release_amd import postprocess as PP, synth
    rng = np.random.default_rng(11)
    B, N = 3, 6000
    pts = synth.make_batch([1, 2, 3], N)
    pred = {"score": rng.standard_normal((B, 3, N)).astype(np.float32) * 3,
            "frame_R": rng.standard_normal((B, 9, N)).astype(np.float32),
            "frame_t": rng.standard_normal((B, 4, N)).astype(np.float32)}
    cam = np.linalg.qr(rng.standard_normal((3, 3)))[0]                 # a camera2base rotation
    dm = cam @ OP.TRAIN2REAL[:3, :3]                                   # grasp_detector.py:155
    thr, vthr = 0.8, 0.2
    H, s, idx, cnt = PP.detect_poses({k: torch.from_numpy(v).to(dev) for k, v in pred.items()},
                                     torch.from_numpy(pts).to(dev), thr, vthr, direction_matrix=dm,
                                     max_poses=2048)
    assert tuple(H.shape) == (B, 2048, 4, 4) and cnt.dtype == torch.int64
    for b in range(B):
        one = {k: v[b] for k, v in pred.items()}
        rH, rs, ridx = OP.detector_post_processing(one, pts[b], thr, vthr, dm)
        n = int(cnt[b])
        assert n == len(ridx) and 0 < n < 2048
        assert np.array_equal(idx[b, :n].cpu().numpy(), ridx)          # same survivors, best first
        assert np.allclose(s[b, :n].cpu().numpy(), rs, atol=2e-6)
        assert np.allclose(H[b, :n].cpu().numpy(), rH, atol=3e-5)
        assert (idx[b, n:] == -1).all() and (H[b, n:] == 0).all() and (s[b, n:] == 0).all()
        assert (np.diff(s[b, :n].cpu().numpy()) <= 0).all()
    # nothing survives an impossible threshold; the cap truncates the best-first list
    H0, s0, i0, c0 = PP.detect_poses({k: torch.from_numpy(v).to(dev) for k, v in pred.items()},
                                     torch.from_numpy(pts).to(dev), 1.5, vthr, direction_matrix=dm)
    assert int(c0.sum()) == 0 and (i0 == -1).all()
    H5, s5, i5, c5 = PP.detect_poses({k: torch.from_numpy(v).to(dev) for k, v in pred.items()},
                                     torch.from_numpy(pts).to(dev), thr, vthr, direction_matrix=dm, max_poses=5)
    assert (c5 == 5).all() and torch.equal(i5, idx[:, :5])


def test_importance_sampling_matches_oracle(dev):
    """grasp_detector.py:237-251 with the uniform draws shared between both sides."""
    from oracle import postprocess as OP
    from s4g_release_amd import postprocess as PP
    rng = np.random.default_rng(3)
    B, K, S = 4, 300, 5
    score = torch.from_numpy(np.sort(rng.random((B, K)).astype(np.float32), axis=1)[:, ::-1].copy()).to(dev)
    count = torch.tensor([300, 120, 5, 3], device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    pick = PP.importance_sampling(score, count, S, generator=g)
    g = torch.Generator(device=dev).manual_seed(7)
    u = torch.rand((B, S), generator=g, device=dev, dtype=torch.float64).cpu().numpy()
    for b in range(2):
        n = int(count[b])
        ref = OP.importance_sampling(score[b, :n].cpu().numpy().astype(np.float64), u[b])
        assert np.array_equal(pick[b].cpu().numpy(), ref)
    assert pick[2].cpu().tolist() == [0, 1, 2, 3, 4] and pick[3].cpu().tolist() == [0, 1, 2, -1, -1]


# ---------------------------------------------------------------------------
# Against fixtures the REFERENCE'S OWN functions produced (tools/gen_golden_post.py)
# ---------------------------------------------------------------------------
import os

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_detect_poses_reference_indexing_equals_the_reference(dev, case):
    """`detect_poses(..., reference_indexing=True)` against what `GraspDetector.post_processing`
    (grasp_detector.py:137-185) itself returned for the same head tensors: same number of poses,
    same point order, same scores, same 4x4 frames (fp32 decode vs the reference's float64)."""
    from s4g_release_amd import postprocess as PP
    fx = np.load(os.path.join(_GOLDEN, "post_detector.npz"))
    pred = {k: torch.from_numpy(fx["%s_%s" % (case, k)]).to(dev) for k in ("score", "frame_R", "frame_t")}
    pts = torch.from_numpy(fx[case + "_points"]).to(dev).unsqueeze(0)
    sthr, vthr = fx[case + "_thresholds"]
    H, s, idx, cnt = PP.detect_poses(pred, pts, float(sthr), float(vthr), direction_matrix=fx["direction_matrix"],
                                     frame=fx["train2real"], max_poses=1024, reference_indexing=True)
    ref_H, ref_s = fx[case + "_mat44"], fx[case + "_scores"]
    n = int(cnt[0])
    assert n == ref_H.shape[0]
    assert np.allclose(s[0, :n].cpu().numpy(), ref_s, atol=1e-6)
    assert np.allclose(H[0, :n].cpu().numpy(), ref_H, atol=3e-5)
    assert (idx[0, n:] == -1).all() and (H[0, n:] == 0).all()
    if n > 1:
        assert (np.diff(idx[0, :n].cpu().numpy()) > 0).all()      # the reference's order: by point index


def test_detect_poses_reference_indexing_batches_like_single_scenes(dev):
    """The reference only accepts B == 1 (grasp_detector.py:49); the batched call is the per-scene
    call scene by scene, and the default (corrected) pairing is a different function."""
    from s4g_release_amd import postprocess as PP
    fx = np.load(os.path.join(_GOLDEN, "post_detector.npz"))
    n = 2048
    pred = {k: torch.from_numpy(np.concatenate([fx["c_" + k], fx["a_" + k][:, :, :n]])).to(dev)
            for k in ("score", "frame_R", "frame_t")}
    pts = torch.from_numpy(np.stack([fx["c_points"], fx["a_points"][:, :n]])).to(dev)
    sthr, vthr = fx["c_thresholds"]
    kw = dict(direction_matrix=fx["direction_matrix"], frame=fx["train2real"], max_poses=512)
    H, s, idx, cnt = PP.detect_poses(pred, pts, float(sthr), float(vthr), reference_indexing=True, **kw)
    assert int(cnt[0]) == fx["c_mat44"].shape[0]
    assert np.allclose(H[0, :int(cnt[0])].cpu().numpy(), fx["c_mat44"], atol=3e-5)
    one = {k: v[1:2] for k, v in pred.items()}
    H1, s1, i1, c1 = PP.detect_poses(one, pts[1:2], float(sthr), float(vthr), reference_indexing=True, **kw)
    assert torch.equal(H[1], H1[0]) and torch.equal(idx[1], i1[0]) and int(cnt[1]) == int(c1[0])
    Hd, sd, idd, cd = PP.detect_poses(pred, pts, float(sthr), float(vthr), **kw)
    assert not torch.equal(idd[0], idx[0])                          # best-first vs point order


@pytest.mark.parametrize("case", ["a", "b"])
def test_collision_check_equals_the_reference_verdicts(dev, case):
    """`view_non_collision(inverse="se3")` against the verdicts of the reference's
    `CloudCollisionChecker.view_non_collision` fed by `torch_batch_transformation_inv`
    (grasp_detector.py:216-225): 96 poses near a 25 600- / 8 000-point cloud."""
    from oracle import postprocess as OP
    from s4g_release_amd import postprocess as PP
    cx = np.load(os.path.join(_GOLDEN, "post_collision.npz"))
    poses = torch.from_numpy(cx[case + "_poses"]).float().to(dev).unsqueeze(0)
    cloud = torch.from_numpy(cx[case + "_cloud"]).to(dev).unsqueeze(0)
    assert np.allclose(PP.se3_inverse(poses)[0].cpu().numpy(), cx[case + "_global2local"], atol=1e-6)
    ok, counts = PP.view_non_collision(poses, cloud, inverse="se3")
    ok = ok[0].cpu().numpy()
    ref_ok = cx[case + "_ok"]
    # a verdict may only differ where a count sits at its threshold (a point within rounding of a
    # box face moves the count by one): name those poses through the oracle's counts
    _, rc = OP.view_non_collision(cx[case + "_poses"][None], cx[case + "_cloud"][None],
                                  global2local=cx[case + "_global2local"][None])
    _, back_thr, finger_thr = cx["thresholds"]
    edge = (np.abs(rc[0, :, 0] - back_thr) <= 1.0) | (np.abs(rc[0, :, 1] - finger_thr) <= 1.0)
    assert np.array_equal(ok[~edge], ref_ok[~edge])
    assert (ok == ref_ok).mean() >= 0.97 and 0 < ref_ok.sum() < ref_ok.size
    assert np.abs(counts[0].cpu().numpy().astype(np.int64) - rc[0]).max() <= 2


@pytest.mark.parametrize("case", ["a", "b"])
def test_demo_decode_and_filter_equal_the_reference(dev, case):
    """`decode_top_poses(..., "demo")` + `view_non_collision` (the product's counterpart of the demo's
    `loggin_to_file(with_label=False)`, utils/file_logger_cls.py:27-47,66-68,196-241) against what the
    reference's own function returned: the same viable frames in the same order, scores to 1e-6, frames
    to 3e-5 (fp32 decode on the device vs fp32 / float64 numpy)."""
    from oracle import postprocess as OP
    from s4g_release_amd import postprocess as PP
    dx = np.load(os.path.join(_GOLDEN, "post_demo.npz"))
    pred_np = {k: dx["%s_%s" % (case, k)] for k in ("score", "frame_R", "frame_t")}
    pred = {k: torch.from_numpy(v).to(dev) for k, v in pred_np.items()}
    pts = torch.from_numpy(dx[case + "_points"]).to(dev)
    H, s, idx = PP.decode_top_poses(pred, pts, 50, "demo")
    ok, counts = PP.view_non_collision(H, pts)                     # float64 inverse, like the demo's caller
    ref_H, ref_s = dx[case + "_top_H"], dx[case + "_top_score"]
    # the reference's 50 candidates, its verdicts and counts through the pinned oracle
    oH, os_, oi = OP.decode_top_poses(pred_np, dx[case + "_points"], K=50)
    assert np.array_equal(idx[0].cpu().numpy(), oi[0])             # same 50 points, best first
    _, rc = OP.view_non_collision(oH.astype(np.float64), dx[case + "_points"])
    edge = (np.abs(rc[0, :, 0] - 10 * np.sqrt(8)) <= 1.0) | (np.abs(rc[0, :, 1] - 10) <= 1.0)
    _, _, ref_idx = OP.demo_top_frames(pred_np, dx[case + "_points"], 50)
    ref_ok = np.isin(oi[0], ref_idx)
    got_ok = ok[0].cpu().numpy()
    assert np.array_equal(got_ok[~edge], ref_ok[~edge]) and 0 < ref_ok.sum() < 50
    both = got_ok & ref_ok
    assert np.allclose(s[0].cpu().numpy()[both], ref_s[np.isin(ref_idx, oi[0][both])], atol=1e-6)
    assert np.allclose(H[0].cpu().numpy()[both], ref_H[np.isin(ref_idx, oi[0][both])], atol=3e-5)


# ---- expected score and pose decode at their edges: tail blocks (N not a multiple of 256, K not a multiple of 64),
# C = 1 .. 8 classes, logits that overflow a softmax without the max subtracted, ties, 1 .. 4 t bins, nearly parallel
# frame columns of any magnitude; all against float64 restatements

@pytest.mark.parametrize("C", [1, 2, 3, 5, 8])
def test_expected_score_edges(dev, C):
    from s4g_release_amd import postprocess as PP
    rng = np.random.default_rng(C)
    worst = 0.0
    for B in (1, 4):
        for N in (1, 255, 256, 257, 25600):
            lg = rng.standard_normal((B, C, N)) * 3
            big = rng.random((B, N)) < 0.3                                       # logits up to +-1e3
            lg = np.where(big[:, None], rng.uniform(-1e3, 1e3, (B, C, N)), lg)
            tie = rng.random((B, N)) < 0.1                                       # every class the same logit
            lg = np.where(tie[:, None], rng.choice([-1e3, -7.5, 0.0, 1e3], (B, 1, N)), lg)
            if C > 1:                                                            # two tied maxima
                two = rng.random((B, N)) < 0.1
                top = lg.max(axis=1) + rng.uniform(0, 1e3, (B, N))
                lg[:, 0] = np.where(two, top, lg[:, 0])
                lg[:, C - 1] = np.where(two, top, lg[:, C - 1])
            lg = lg.astype(np.float32)
            for convention in ("demo", "detector"):
                got = PP.expected_score(torch.from_numpy(lg).to(dev), convention).cpu().numpy().astype(np.float64)
                v = np.linspace(0, 1, C + 1)
                v = v[:-1] if convention == "demo" else v[1:]
                ref = (torch.softmax(torch.from_numpy(lg).double(), dim=1).numpy() * v[None, :, None]).sum(1)
                assert np.isfinite(got).all(), (B, N, convention)
                worst = max(worst, float(np.abs(got - ref).max()))
    # fp32 exp / sum / divide of at most 8 terms, output in [0, 1]: a few eps (6e-8) each; measured on the MI355X at
    # most 2.1e-7 (C = 8), 1.2e-7 (C = 2), 0 (C = 1)
    print("expected_score C=%d: max |err| %.3g (bound 1e-6)" % (C, worst))
    assert worst < 1e-6


def _frames(rng, B, N):
    """(B, 9, N) row-major frames whose first two columns meet at angles from 1e-2 to pi - 1e-2 rad with magnitudes
    1e-3 .. 1e3 each (third column arbitrary: the decode ignores it), and the angles (B, N)."""
    ang = rng.choice([1e-2, 2e-2, 0.1, 0.5, 1.2, np.pi / 2, np.pi - 0.1, np.pi - 1e-2], (B, N))
    u = rng.standard_normal((B, N, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    w = rng.standard_normal((B, N, 3))
    w -= (u * w).sum(-1, keepdims=True) * u
    w /= np.linalg.norm(w, axis=-1, keepdims=True)
    c0 = u * 10 ** rng.uniform(-3, 3, (B, N, 1))
    c1 = (np.cos(ang)[..., None] * u + np.sin(ang)[..., None] * w) * 10 ** rng.uniform(-3, 3, (B, N, 1))
    c2 = rng.standard_normal((B, N, 3)) * 10 ** rng.uniform(-3, 3, (B, N, 1))
    R = np.stack([c0, c1, c2], axis=-1)                                          # (B, N, 3, 3), columns c0 c1 c2
    return np.ascontiguousarray(R.reshape(B, N, 9).transpose(0, 2, 1)).astype(np.float32), ang


@pytest.mark.parametrize("K", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("TC", [1, 2, 3, 4])
def test_decode_top_poses_edges(dev, K, TC):
    from s4g_release_amd import postprocess as PP
    rng = np.random.default_rng(K * 10 + TC)
    B, N = 2, 300
    R, ang = _frames(rng, B, N)
    pred = {"score": rng.standard_normal((B, 3, N)).astype(np.float32) * 2, "frame_R": R,
            "frame_t": (rng.standard_normal((B, TC, N)) * 4).astype(np.float32)}
    pts = rng.uniform(-1, 1, (B, 3, N)).astype(np.float32)
    H, s, sel = PP.decode_top_poses({k: torch.from_numpy(v).to(dev) for k, v in pred.items()},
                                    torch.from_numpy(pts).to(dev), K)
    H, s, sel = H.cpu().numpy().astype(np.float64), s.cpu().numpy(), sel.cpu().numpy()
    assert H.shape == (B, K, 4, 4)
    # the selection: the K best expected scores, best first
    es = (torch.softmax(torch.from_numpy(pred["score"]).double(), dim=1).numpy() *
          np.linspace(0, 1, 4)[:-1][None, :, None]).sum(1)
    assert np.allclose(s, np.take_along_axis(es, sel, 1), atol=1e-6) and (np.diff(s, axis=1) <= 0).all()
    assert np.array_equal(np.sort(sel, 1), np.sort(np.argsort(-es, 1)[:, :K], 1))
    # float64 Gram-Schmidt and translation decode of the selected points' fp32 inputs
    Rk = np.take_along_axis(R.astype(np.float64), sel[:, None, :], 2).transpose(0, 2, 1).reshape(B, K, 3, 3)
    c0, c1 = Rk[..., 0], Rk[..., 1]
    x = c0 / np.linalg.norm(c0, axis=-1, keepdims=True)
    y = c1 - (x * c1).sum(-1, keepdims=True) * x
    y /= np.linalg.norm(y, axis=-1, keepdims=True)
    R64 = np.stack([x, y, np.cross(x, y)], axis=-1)
    tl = np.take_along_axis(pred["frame_t"].astype(np.float64), sel[:, None, :], 2)
    tau = (torch.softmax(torch.from_numpy(tl), dim=1).numpy() * np.array(PP.T_BINS[:TC])[None, :, None]).sum(1)
    p = np.take_along_axis(pts.astype(np.float64), sel[:, None, :], 2).transpose(0, 2, 1)
    t64 = -tau[..., None] * c0 + p
    # rotation: the direction of y carries the projection's rounding, ~eps |c1| / (|c1| sin a) -- float32 emulation
    # of the kernel's arithmetic gives at most 1.9e-7 / sin(a) over angles 1e-2 .. pi/2; measured on the MI355X at
    # most 1.7e-7 / sin(a) over these cases
    sin = np.sin(np.take_along_axis(ang, sel, 1))
    r_err = np.abs(H[..., :3, :3] - R64).max(axis=(-1, -2)) * sin
    # translation: fp32 softmax of <= 4 bins, one product, one sum: a few eps of |tau c0| + |p|; measured at most
    # 1.9e-7 of that scale
    t_err = np.abs(H[..., :3, 3] - t64).max(-1) / (np.abs(tau[..., None] * c0).max(-1) + np.abs(p).max(-1))
    print("decode K=%d TC=%d: rotation err * sin(a) %.3g (bound 1e-6), translation err / scale %.3g (bound 1e-6)"
          % (K, TC, r_err.max(), t_err.max()))
    assert r_err.max() < 1e-6 and t_err.max() < 1e-6
    # orthonormal even at a = 1e-2: one Gram-Schmidt projection alone leaves x.y ~ eps / sin(a), 3.4e-5 in the float32
    # emulation -- the kernel projects twice (emulation: at most 5.5e-7 over all angles)
    RtR = np.einsum("bkij,bkil->bkjl", H[..., :3, :3], H[..., :3, :3])
    assert np.abs(RtR - np.eye(3)).max() < 1e-5
    assert np.abs(np.linalg.det(H[..., :3, :3]) - 1).max() < 1e-5                 # right-handed
    assert (H[..., 3, :] == np.array([0, 0, 0, 1])).all()
