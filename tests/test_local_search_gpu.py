"""The data generator's local grasp search on the device (`postprocess.grade_local_search`, csrc/local_search.hip; the
reference's `TorchSingleViewPointCloud.finger_hand`, data_gen/pcd_classes/torch_single_view_point_cloud.py:224-358)
against the fixture the reference produced (tests/golden/local_search.npz), the float64 yardstick and the exact
constructions of tests/local_search_ref.py (checked on the CPU by tests/test_local_search_ref.py) and the
`eval_frames` route on the composed poses.

Score tolerance: 1e-4 of float64 (the bound tests/test_eval_frames_gpu.py uses for this same score, scale 1)."""
import numpy as np
import pytest
import torch

from tests import golden_util as GU
from tests import local_search_ref as LR

pytestmark = pytest.mark.gpu

FIELDS = ("search_score", "objects_label", "back", "finger", "close", "table_collision", "antipodal_score",
          "slab_count", "valid", "valid_index", "count")


def _t(a, dev):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(dev, points, frames, cloud, normals, labels, cfg=None, count=None):
    from s4g_release_amd import postprocess as PP
    return PP.grade_local_search(_t(points, dev), _t(frames, dev), _t(cloud, dev), _t(normals, dev), _t(labels, dev), cfg,
                                 None if count is None else torch.as_tensor(count).to(dev))


def _np(r):
    return {k: getattr(r, k).cpu().numpy() for k in FIELDS}


def _same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("ints", "slab_count", "valid_i32", "valid_index", "count")) \
        and torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32))


def _cfg(**kw):
    from s4g_release_amd.postprocess import LocalSearchConfig
    return LocalSearchConfig(**kw)


def _fixture():
    fx = GU.load("local_search.npz")
    return fx, (fx["points"], fx["frames"], fx["cloud"], fx["normals"], fx["labels"])


def _check_against_yardstick(got, y, what, live=None):
    """One scene: `got` the call's arrays, `y` = `search64`.  On decided frames every integer and flag is the
    yardstick's and the scores are within SCORE_TOL; slab counts within the points that sit on a slab bound; frames
    that fail a gate or are padding read 0 / no_label / False."""
    ok = LR.decided(y) if live is None else LR.decided(y) & live
    for k in ("search_score", "objects_label", "table_collision", "valid"):
        assert np.array_equal(got[k][ok], y[k][ok]), (what, k)
    err = np.abs(got["antipodal_score"].astype(np.float64) - y["antipodal_score"])[ok]
    print("%s: max |score - float64| = %.3g over %d decided frames" % (what, err.max() if err.size else 0.0, int(ok.sum())))
    assert (err <= LR.SCORE_TOL).all(), (what, err.max())
    assert (np.abs(got["slab_count"] - y["slab_count"]) <= y["amb_slab"])[ok].all(), what
    # the three counts behind the verdicts, wherever no point sits within the tolerance of a face of the placement's regions
    clear = (ok & y["gate"])[:, None, None] & y["clear"]
    for k in ("back", "finger", "close"):
        assert np.array_equal(got[k][clear], y[k][clear]), (what, k)
    dead = ~y["gate"] & LR.decided(y)
    for k in ("search_score", "back", "finger", "close", "table_collision", "antipodal_score", "slab_count", "valid"):
        assert not got[k][dead].any(), (what, k)
    # the compaction is that of the call's own validity, whatever the frames
    vi = np.nonzero(got["valid"])[0]
    assert got["count"] == len(vi) and np.array_equal(got["valid_index"][:len(vi)], vi)
    assert (got["valid_index"][len(vi):] == -1).all()


def test_fixture_of_the_reference(dev):
    """Every integer / bool output equals the reference's, scores within 1e-4 of float64 and within 1e-4 + margin of
    the reference, valid_index / count equal, frames_of within 1e-5."""
    fx, d = _fixture()
    r = _run(dev, *d)
    got = {k: v[0] for k, v in _np(r).items()}
    assert np.array_equal(got["search_score"], fx["search_score"])
    assert np.array_equal(got["objects_label"], fx["objects_label"])
    assert np.array_equal(got["valid"], fx["valid"])
    y = LR.search64(*d, _cfg())
    assert LR.decided(y).all()
    e64 = np.abs(got["antipodal_score"].astype(np.float64) - y["antipodal_score"]).max()
    efx = np.abs(got["antipodal_score"].astype(np.float64) - fx["antipodal_score"]).max()
    print("fixture: max |score - float64| = %.3g, |score - reference| = %.3g" % (e64, efx))
    assert e64 <= LR.SCORE_TOL and efx <= LR.SCORE_TOL + float(fx["margin"][0])
    vi = np.nonzero(fx["valid"])[0]
    assert got["count"] == len(vi) and np.array_equal(got["valid_index"][:len(vi)], vi)
    assert (got["valid_index"][len(vi):] == -1).all()
    vf = r.frames_of()[0, :len(vi)].cpu().numpy()
    assert np.abs(vf - fx["valid_frame"][vi]).max() <= 1e-5
    _check_against_yardstick(got, y, "fixture")
    dump = r.dump(0)
    assert np.array_equal(dump["search_score"], fx["search_score"][vi]) and dump["objects_label"].dtype == np.int16
    assert np.array_equal(dump["valid_index"], vi) and np.abs(dump["valid_frame"] - fx["valid_frame"][vi]).max() <= 1e-5


P = LR.FRAMES_PER_PASS
# N around a wave, a sweep of 1 024 points (in one chunk of four: 4 x 1 024 +- 1) and the chunk count's turn
# (4 x 16 384 +- 1: four and five chunks); F around the 256 frames of a pass; B of 1 and 3 with a different frame_count
# per scene, 0 among them.  Every shape has at least two frames, so that the zero frame is never the only one.
EDGES = [(1, 1, 2), (1, 63, 2), (1, 64, P - 1), (3, 65, P), (1, 1023, P + 1), (3, 1025, 3), (1, 4095, 2), (1, 4097, 3),
         (1, 65535, 3), (1, 65537, 2)]


def _edge_case(B, N, F):
    """The scenes of an EDGES shape (seeded by it) and, per scene, the yardstick on all F frames.  Frame F // 2 of the
    first scene is the zero frame where there are three frames or more."""
    cfg = _cfg()
    rng = np.random.default_rng(N * 7 + F)
    scenes = [LR.blob_scene(rng, N, F, cfg) for _ in range(B)]
    d = [np.stack([s[i] for s in scenes]) for i in range(5)]
    if F >= 3:
        d[1][0, F // 2] = 0
    ys = {(b, F): LR.search64(d[0][b], d[1][b], d[2][b], d[3][b], d[4][b], cfg) for b in range(B)}
    for b in range(B):                                  # the shape checks something: live, decided frames in every scene,
        live = LR.decided(ys[(b, F)]) & ys[(b, F)]["gate"]                   # scored placements from N = 63 on
        assert live.sum() > 0, (B, N, F, b)
        assert N < 63 or ((ys[(b, F)]["reason"] == 0) & live[:, None, None]).sum() > 0, (B, N, F, b)
        assert ys[(b, F)]["slab_count"][live].max() > 0
    return cfg, d, ys


@pytest.mark.parametrize("B,N,F", EDGES)
def test_loop_edges_against_the_yardstick(dev, B, N, F):
    cfg, d, ys = _edge_case(B, N, F)
    cnt = np.array([F, (F + 1) // 2, 0][:B])
    for count in (None, cnt):
        got = _np(_run(dev, *d, cfg, count))
        for b in range(B):
            n = F if count is None else int(count[b])
            if (b, n) not in ys:
                ys[(b, n)] = LR.search64(d[0][b], d[1][b], d[2][b], d[3][b], d[4][b], cfg, frame_count=n)
            _check_against_yardstick({k: v[b] for k, v in got.items()}, ys[(b, n)], "edge %s scene %d" % ((B, N, F), b))


@pytest.mark.parametrize("kw", [dict(length_search=(-0.04,)), dict(theta_search_deg=(30,)),
                                dict(length_search=(-0.06,), theta_search_deg=(-45,)), dict()])
def test_one_depth_one_angle_and_the_reference_shape(dev, kw):
    cfg = _cfg(**kw)
    fx, d = _fixture()
    d = [a[:40] if i < 2 else a for i, a in enumerate(d)]
    got = {k: v[0] for k, v in _np(_run(dev, *d, cfg)).items()}
    assert got["search_score"].shape == (40,) + cfg.shape
    _check_against_yardstick(got, LR.search64(*d, cfg), "shape %s" % (cfg.shape,))


def test_points_on_the_faces_slab_bounds_and_band_bounds(dev):
    """Exact fp32 coordinates: points on, one ulp inside and one ulp outside every bound count exactly (strict
    inequalities), and the score tells the band populations (the points on the band bounds carry |n.y| = 1)."""
    cfg = LR.face_config()
    d = LR.face_scene(cfg)
    y = LR.search64(*d, cfg, band_f32=True)
    got = {k: v[0] for k, v in _np(_run(dev, *d, cfg)).items()}
    for k in ("back", "finger", "close", "search_score", "objects_label", "slab_count", "table_collision", "valid"):
        assert np.array_equal(got[k], y[k]), k
    assert (y["reason"] == 0).all() and (y["close"] > 4).all()
    assert np.abs(got["antipodal_score"] - y["antipodal_score"]).max() <= 1e-6


def test_all_invalid_and_a_single_valid_frame_at_the_last_row(dev):
    fx, d = _fixture()
    dead = np.nonzero(~fx["valid"])[0]
    one = np.nonzero(fx["valid"])[0][:1]
    r = _run(dev, fx["points"][dead], fx["frames"][dead], *d[2:])
    assert int(r.count[0]) == 0 and bool((r.valid_index == -1).all()) and not bool(r.valid.any())
    sel = np.concatenate([dead, one])
    r = _run(dev, fx["points"][sel], fx["frames"][sel], *d[2:])
    assert int(r.count[0]) == 1 and int(r.valid_index[0, 0]) == len(sel) - 1 and bool((r.valid_index[0, 1:] == -1).all())


def _batch(dev, B=3, N=12000, seed=5):
    """Three different subsamples of the fixture's scene with the fixture's frames in three different orders."""
    fx, d = _fixture()
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.permutation(d[2].shape[1])[:N] for _ in range(B)])
    order = np.stack([rng.permutation(len(d[0])) for _ in range(B)])
    return [_t(a, dev) for a in (np.stack([d[0][o] for o in order]), np.stack([d[1][o] for o in order]),
                                 np.stack([d[2][:, i] for i in idx]), np.stack([d[3][:, i] for i in idx]),
                                 np.stack([d[4][i] for i in idx]))]


def test_two_calls_are_bit_identical_and_a_scene_alone_equals_it_in_a_batch(dev):
    d = _batch(dev)
    cnt = torch.tensor([150, 100, 17], device=dev)
    a = _run(dev, *d, None, cnt)
    assert int((a.antipodal_score > 0).sum()) > 20 and int(a.count.sum()) > 8
    for _ in range(2):
        assert _same(a, _run(dev, *d, None, cnt))
    for b in range(3):
        one = _run(dev, *[t[b:b + 1].contiguous() for t in d], None, cnt[b:b + 1])
        assert torch.equal(one.ints[0], a.ints[b]) and torch.equal(one.scores[0].view(torch.int32),
                                                                   a.scores[b].view(torch.int32)), b
        assert torch.equal(one.valid_index[0], a.valid_index[b]) and torch.equal(one.slab_count[0], a.slab_count[b])


def test_graph_capture_and_replay(dev):
    d = _batch(dev)
    cnt = torch.tensor([150, 120, 60], device=dev)
    eager = _run(dev, *d, None, cnt)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        _run(dev, *d, None, cnt)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _run(dev, *d, None, cnt)
    for _ in range(2):
        for t in (out.ints, out.scores, out.slab_count, out.valid_i32, out.valid_index, out.count):
            t.zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        assert _same(out, eager)


def test_a_scene_with_nan_coordinates_is_contained(dev):
    """One scene of the batch holds NaN and inf coordinates and normals: the call returns and the clean scenes' outputs
    are bit-identical to a run without that scene (its own outputs are unspecified)."""
    d = _batch(dev)
    clean = _run(dev, *[t[[0, 2]].contiguous() for t in d])
    d[2][1, 0, 77::5] = float("nan")
    d[2][1, 2, 1000] = float("inf")
    d[3][1, 1, 50:600] = float("nan")
    d[0][1, 3, 1] = float("nan")
    bad = _run(dev, *d)
    torch.cuda.synchronize(dev)
    for i, b in enumerate((0, 2)):
        assert torch.equal(bad.ints[b], clean.ints[i])
        assert torch.equal(bad.scores[b].view(torch.int32), clean.scores[i].view(torch.int32))
        assert torch.equal(bad.valid_index[b], clean.valid_index[i]) and bad.count[b] == clean.count[i]


def test_the_eval_frames_route_gives_the_same_verdicts(dev):
    """`eval_frames` on the L * T composed poses [R | p] @ LOCAL_SEARCH_TO_LOCAL with inverse="se3": on decided frames
    the counts behind the palm / in the fingers / in the close region and the multi-object flag are equal wherever the
    slab gate and the table gate let the placement through, and the scores are within 2e-4."""
    from s4g_release_amd import postprocess as PP
    cfg = _cfg()
    fx, d = _fixture()
    y = LR.search64(*d, cfg)
    r = _run(dev, *d, cfg)
    L, T = cfg.shape
    F = len(d[0])
    poses = LR.composed_poses(d[0], d[1], cfg).reshape(1, F * L * T, 4, 4)
    poses[~np.isfinite(poses)] = 0
    g = PP.GripperConfig(half_bottom_width=cfg.half_bottom_width, bottom_length=cfg.bottom_length,
                         finger_width=cfg.finger_width, half_hand_thickness=cfg.half_hand_thickness,
                         finger_length=cfg.finger_length, back_collision_margin=cfg.back_collision_margin,
                         back_collision_threshold=cfg.back_collision_threshold,
                         finger_collision_threshold=cfg.finger_collision_threshold,
                         close_region_min_points=cfg.close_region_min_points, neighbor_depth=cfg.neighbor_depth)
    e = PP.eval_frames(_t(poses, dev), _t(d[2][None], dev), _t(d[3][None], dev), _t(d[4][None], dev), g, inverse="se3")
    # The counts are compared on placements with no scene point within 1.5e-6 of a face of the placement's regions: the
    # two routes round a point's local coordinates differently (the composed pose's matrix entries and its inverse's
    # translation are rounded once more), each within about 1e-6 of float64 here -- three products of magnitude up to
    # 1.3 and a translation up to 1.5, every one rounded to an fp32 ulp of 1.2e-7 to 2.4e-7 -- so a point nearer than
    # that to a face may count on one route and not on the other.  That leaves three quarters of the placements.
    every = (LR.decided(y) & y["gate"])[:, None, None] & ~y["table_collision"] & (y["slab_count"] >= 8)[:, :, None]
    through = every & LR.search64(*d, cfg, clear_tol=1.5e-6)["clear"]
    print("eval_frames route: %d of %d placements past the table and slab gates are compared" % (through.sum(), every.sum()))
    assert through.sum() >= 0.7 * every.sum()
    assert through.sum() > 500
    view = lambda t: t.cpu().numpy().reshape(F, L, T)
    got = _np(r)
    for k, ek in (("back", e.back), ("finger", e.finger), ("close", e.close)):
        diff = got[k][0][every].astype(np.int64) - view(ek)[every]
        print("eval_frames route: %s differs on %d of all %d placements past the two gates, by at most %d"
              % (k, int((diff != 0).sum()), diff.size, int(np.abs(diff).max())))
    for k, ek in (("back", e.back), ("finger", e.finger), ("close", e.close)):
        assert np.array_equal(got[k][0][through], view(ek)[through]), k
    reach = through & ((y["reason"] == 0) | (y["reason"] == 6))                # past the collision and count gates
    assert np.array_equal(view(e.multi_objects)[reach], (y["reason"] == 6)[reach])
    scored = through & (y["reason"] == 0)
    assert scored.sum() >= 40
    assert np.abs(got["antipodal_score"][0][scored] - view(e.score)[scored]).max() <= 2e-4
    # reaching the score means the same on both routes
    assert np.array_equal((view(e.score) != 0)[through], scored[through])


def test_refuses_cpu_tensors_wrong_shapes_and_a_height_search(dev):
    from s4g_release_amd import postprocess as PP
    fx, d = _fixture()
    t = [_t(a[:4] if i < 2 else a[..., :1000], dev) for i, a in enumerate(d)]
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        PP.grade_local_search(t[0].cpu(), *t[1:])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        PP.grade_local_search(*t[:4], t[4].cpu())
    with pytest.raises(RuntimeError, match="int32"):
        PP.grade_local_search(*t[:4], t[4].long())
    with pytest.raises(RuntimeError, match="scene_normals"):
        PP.grade_local_search(*t[:3], t[3][:, :999].contiguous(), t[4])
    with pytest.raises(RuntimeError, match="frames"):
        PP.grade_local_search(t[0], t[1][:3], *t[2:])
    with pytest.raises(ValueError, match="THICKNESS_SEARCH"):
        PP.grade_local_search(*t, _cfg(thickness_search=(0.01,)))
    with pytest.raises(ValueError, match="depths"):
        PP.grade_local_search(*t, _cfg(length_search=tuple([-0.02] * 9)))
    r = PP.grade_local_search(*t)                                              # unbatched inputs get a leading 1
    assert tuple(r.search_score.shape) == (1, 4, 4, 12) and tuple(r.count.shape) == (1,)
