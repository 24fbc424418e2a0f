"""The curvature model's per-object data on the device (`postprocess.estimate_object_frames`, `grade_object_frames`,
`label_darboux_object`, `compose_darboux_scene`; csrc/darboux.hip, csrc/darboux_object.hip) against the fixture the
reference's own `_estimate_frame` and `finger_hand_view` produced (tests/golden/darboux_object.npz) and the float64
yardstick of tests/darboux_object_ref.py (checked on the CPU by tests/test_darboux_object_ref.py).

Grading.  The counts, the slab counts and `search_score` exact, `antipodal_score` within SCORE_TOL = 1e-4 of float64
(the bar of tests/local_search_ref.py for this same score), each on the rows the yardstick calls decided at the
fixture's own eps0.  The yardstick is run on every third graded frame of the fixture and on its whole sparse cloud.

Frames.  FRAME_FACTOR * margin / g against float64, modulo the joint flip of columns y and z, as tests/test_darboux_gpu.py
holds the view frames: g = (l1 - l0) / l2 is the relative eigenvalue gap of the covariance, on which the eigenvector of
l0 depends with condition 1 / g; `margin` = 4.4e-7 is the fixture's own measure of what fp32 costs here -- the largest
(distance from float64 of an fp32 numpy restatement of :73-91) * g over its decided frames, about 7 ulps of l2 --;
and the kernel gets FRAME_FACTOR = 8 of it because its summation order and its eigen-solver (cyclic Jacobi in fp32 on
the covariance rounded once) are not LAPACK's, each worth a few ulps of l2.  The bound is 3.5e-6 / g.  Measured on the
fixture (printed by test_fixture_frames, recorded in profiles/r21_darboux_object.md): worst err * g = 1.34e-7 over 310
decided rows, for both frame sets.

The edge clouds sit on a 1 / 2048 m lattice with axis-aligned frames at lattice points and rolls at multiples of 90
degrees: every local coordinate is exact in fp32, a roll moves it by at most 4.4e-8 of its partner, and no bound of any
region is within 5e-5 m of a lattice value (tests/test_darboux_object_ref.py asserts it; the palm plane x - dl < 0
needs no margin, an fp32 difference has the exact sign).  So every count, slab count and search score is exact on
EVERY row there; the antipodal score is compared where no close-region point sits on a band bound (the bound
left_y - (left_y - right_y) / 3 can fall on the lattice)."""
import functools

import numpy as np
import pytest
import torch

from tests import darboux_object_ref as DO
from tests import golden_util as GU

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -559038737
FRAME_FACTOR = 8.0
SUB = 3
LATTICE_EPS = 1e-6


def _t(a, dev):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _guarded(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _read(bufs, floats=()):
    out = {}
    for k, (buf, view) in bufs.items():
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "guard of %s" % k
        a = view.cpu().numpy()
        out[k] = a.view(np.float32) if k in floats else a
    return out


def _cf(a):
    """(N, 3) -> (1, 3, N) contiguous"""
    return np.ascontiguousarray(a.T[None])


def _cfg(**kw):
    from s4g_release_amd.postprocess import DarbouxObjectConfig
    return DarbouxObjectConfig(**kw)


def _frames_guarded(dev, xyz, nrm, count=None, cfg=None):
    """s4g_darboux_object_frames_f32 through the C ABI with every output inside a guarded buffer."""
    from s4g_release_amd import _cabi
    from s4g_release_amd import functions as Fn
    cfg = cfg or _cfg()
    B, _, N = xyz.shape
    d_x, d_n = _t(xyz, dev), _t(nrm, dev)
    d_c = None if count is None else _t(np.asarray(count, np.int64), dev)
    bufs = {k: _guarded(s, dev) for k, s in (("frames", (B, N, 3, 3)), ("inv_frames", (B, N, 3, 3)),
                                             ("neighbours", (B, N)), ("flags", (B, N)))}
    nbytes = int(_cabi.lib().s4g_darboux_object_frames_workspace_bytes(B, N))
    ws = torch.full((nbytes + 2 * GUARD * 4,), 0x5A, dtype=torch.uint8, device=dev)
    rc = _cabi.lib().s4g_darboux_object_frames_f32(
        d_x.data_ptr(), d_n.data_ptr(), None if d_c is None else d_c.data_ptr(), B, N, float(cfg.radius),
        int(cfg.min_neighbours), bufs["frames"][1].data_ptr(), bufs["inv_frames"][1].data_ptr(),
        bufs["neighbours"][1].data_ptr(), bufs["flags"][1].data_ptr(), ws[GUARD * 4:].data_ptr(), nbytes, Fn._stream())
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    assert (ws[:GUARD * 4] == 0x5A).all() and (ws[GUARD * 4 + nbytes:] == 0x5A).all(), "guard of the workspace"
    return _read(bufs, floats=("frames", "inv_frames"))


def _grade_guarded(dev, xyz, nrm, frames, inv_frames, cfg, count=None, frame_index=None):
    """s4g_darboux_object_grade_f32 through the C ABI with every output inside a guarded buffer."""
    from s4g_release_amd import _cabi, postprocess as PP
    from s4g_release_amd import functions as Fn
    B, _, N = xyz.shape
    F = frames.shape[1]
    L, T, S = cfg.shape
    d_x, d_n, d_f, d_i = _t(xyz, dev), _t(nrm, dev), _t(frames, dev), _t(inv_frames, dev)
    d_c = None if count is None else _t(np.asarray(count, np.int64), dev)
    d_fi = None if frame_index is None else _t(np.asarray(frame_index, np.int32), dev)
    params, table = PP._object_grade_args(cfg)
    d_t = table.to(dev)
    bufs = {k: _guarded(s, dev) for k, s in (("search", (B, F, 2, L, T)), ("antipodal", (B, F, 2, L, T)),
                                             ("counts", (B, F, 2, L, T, S, 3)), ("slab", (B, F, 2, L)),
                                             ("fail", (B, F, 2)))}
    nbytes = int(_cabi.lib().s4g_darboux_object_grade_workspace_bytes(B, N, F, L, T, S))
    ws = torch.full((nbytes + 2 * GUARD * 4,), 0x5A, dtype=torch.uint8, device=dev)
    rc = _cabi.lib().s4g_darboux_object_grade_f32(
        d_x.data_ptr(), d_n.data_ptr(), None if d_c is None else d_c.data_ptr(), d_f.data_ptr(), d_i.data_ptr(),
        None if d_fi is None else d_fi.data_ptr(), B, N, F, L, T, S, params, d_t.data_ptr(),
        bufs["search"][1].data_ptr(), bufs["antipodal"][1].data_ptr(), bufs["counts"][1].data_ptr(),
        bufs["slab"][1].data_ptr(), bufs["fail"][1].data_ptr(), ws[GUARD * 4:].data_ptr(), nbytes, Fn._stream())
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    assert (ws[:GUARD * 4] == 0x5A).all() and (ws[GUARD * 4 + nbytes:] == 0x5A).all(), "guard of the workspace"
    return _read(bufs, floats=("antipodal",))


def _check_grade(got, b, y, what, exact_integers=False):
    """Object b of a guarded grading against the yardstick result y.  exact_integers: the lattice clouds, where the
    counts and the search score are exact on every row; else on the decided rows."""
    d = y["decided"]
    rows = np.ones_like(d) if exact_integers else d
    assert np.array_equal(got["fail"][b] != 0, y["fail"]), what
    live = ~y["fail"]
    assert np.array_equal(got["slab"][b][live], y["slab_count"][live]) or not exact_integers, what
    assert np.array_equal(got["counts"][b][rows], y["counts"][rows]), what
    assert np.array_equal(got["search"][b][rows], y["search_score"][rows]), what
    ga, ya = got["antipodal"][b].astype(np.float64), y["antipodal_score"]
    err = np.abs(ga - ya)[d]
    worst = float(err.max()) if err.size else 0.0
    assert worst <= DO.SCORE_TOL, (what, worst)
    dead = y["fail"]
    for k in ("search", "antipodal", "counts", "slab"):
        assert not got[k][b][dead].any(), (what, k)
    return worst


def _inv(frames):
    return (frames * np.array([-1, -1, 1], np.float32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _fixture():
    fx = GU.load("darboux_object.npz")
    return {k: fx[k] for k in fx.files}


# ---- the fixture ----

def test_fixture_grading(dev):
    """The fixture's own fp32 frames at every graded point, the whole list in one call; the yardstick on every third."""
    fx = _fixture()
    cfg = _cfg()
    sel = fx["subset"]
    fr = fx["frames"][sel]
    got = _grade_guarded(dev, _cf(fx["points"]), _cf(fx["normals"]), fr[None], _inv(fr)[None], cfg, frame_index=sel[None])
    rows = np.arange(0, len(sel), SUB)
    y = DO.grade64(fx["points"], fx["normals"], fr[rows], _inv(fr[rows]), cfg, index=sel[rows], eps=float(fx["eps0"][0]))
    sub = {k: v[:, rows] for k, v in got.items()}
    worst = _check_grade(sub, 0, y, "fixture")
    d = y["decided"]
    assert d.mean() >= 0.75 and (d & (y["search_score"] > 0)).sum() >= 600 and (d & y["fractional"]).sum() >= 300
    # and the reference's own numbers on every decided row of that third: its fp32 antipodal score is within 3e-7 of
    # float64 (the generator prints it)
    assert np.array_equal(sub["search"][0][d], fx["search_score"][rows][d])
    ref = np.abs(sub["antipodal"][0].astype(np.float64) - fx["antipodal_score"][rows])[d].max()
    print("fixture grading: %d placements, %.1f %% decided, antipodal max |diff| to float64 %.3g, to the reference %.3g"
          % (d.size, 100 * d.mean(), worst, ref))
    assert ref <= DO.SCORE_TOL + 1e-5
    # the rows the yardstick did not run: whatever the reference recorded as positive is positive here too, up to the
    # undecided few
    agree = (got["search"][0] == fx["search_score"]).mean()
    assert agree >= 0.97, agree


def test_fixture_sparse_cloud(dev):
    """The thinned cloud: slab skips and close regions with too few points."""
    fx = _fixture()
    cfg = _cfg()
    sp = fx["sparse"]
    fr = fx["frames"][sp]
    got = _grade_guarded(dev, _cf(fx["points"][sp]), _cf(fx["normals"][sp]), fr[None], _inv(fr)[None], cfg)
    y = DO.grade64(fx["points"][sp], fx["normals"][sp], fr, _inv(fr), cfg, eps=float(fx["eps0"][0]))
    _check_grade(got, 0, y, "sparse")
    d = y["decided"]
    assert np.array_equal(got["search"][0][d], fx["sparse_search_score"][d])
    assert {"slab", "few"} <= {DO.OUTCOMES[o] for o in np.unique(y["outcome"][d])}


@pytest.fixture(scope="module")
def fixture_frames(dev):
    fx = _fixture()
    return _frames_guarded(dev, _cf(fx["points"]), _cf(fx["normals"]))


def test_fixture_frames(dev, fixture_frames):
    fx = _fixture()
    got = fixture_frames
    N = len(fx["points"])
    rows = np.arange(0, N, 8)
    y = DO.frames64(fx["points"], fx["normals"], rows=rows)
    kept = np.zeros(N, bool)
    kept[rows] = True
    sure = kept & ~y["near"]
    assert np.array_equal(got["neighbours"][0][sure], y["count"][sure])
    assert (got["neighbours"][0] == fx["neighbours"]).mean() >= 0.999           # (a point on the sphere may count either way)
    ok = kept & DO.frames_decided(y)
    assert ok.sum() >= 250 and (got["flags"][0][ok] == 1).all()
    margin = float(fx["margin"][0])
    for name in ("frames", "inv_frames"):
        err = DO.flip_distance(got[name][0], y[name])
        worst = float((err * y["gap"])[ok].max())
        print("%s: %d decided rows, worst err * g = %.3g (allowed %.3g), worst err %.3g"
              % (name, int(ok.sum()), worst, FRAME_FACTOR * margin, float(err[ok].max())))
        assert (err[ok] <= FRAME_FACTOR * margin / y["gap"][ok]).all(), (name, worst)
    # against the reference's frames: the same bound plus the reference's own distance from float64
    ref = DO.flip_distance(fx["frames"], y["frames"])
    err = DO.flip_distance(got["frames"][0], fx["frames"])
    assert (err[ok] <= FRAME_FACTOR * margin / y["gap"][ok] + ref[ok] + 6e-8).all()
    # every estimated frame is a rotation with the pinned sign; the opposite frame negates x and y exactly
    est = got["flags"][0] == 1
    assert est.sum() >= 0.9 * N
    Q = got["frames"][0][est].astype(np.float64)
    assert np.abs(Q.transpose(0, 2, 1) @ Q - np.eye(3)).max() <= 1e-5 and np.abs(np.linalg.det(Q) - 1).max() <= 1e-5
    assert np.array_equal(got["inv_frames"][0], got["frames"][0] * np.array([-1, -1, 1], np.float32))
    z = Q[:, :, 2]
    top = np.take_along_axis(z, np.abs(z).argmax(1)[:, None], 1)[:, 0]
    assert ((top > 0) | (np.abs(top) - np.sort(np.abs(z), 1)[:, 1] <= 1e-6)).all()


def test_label_is_the_two_stages_and_dump(dev, fixture_frames):
    from s4g_release_amd import postprocess as PP
    fx = _fixture()
    xyz, nrm = _t(_cf(fx["points"]), dev), _t(_cf(fx["normals"]), dev)
    lab = PP.label_darboux_object(xyz, nrm)
    fr = PP.estimate_object_frames(xyz, nrm)
    gr = PP.grade_object_frames(xyz, nrm, fr.frames, fr.inv_frames)
    for k in ("frames", "inv_frames", "neighbours", "flags"):
        assert torch.equal(getattr(lab.frames, k).view(torch.int32), getattr(fr, k).view(torch.int32)), k
        assert np.array_equal(getattr(fr, k).cpu().numpy().view(np.int32), fixture_frames[k].view(np.int32)), k
    for k in ("search_score", "antipodal_score", "counts", "slab_count", "fail_i32"):
        assert torch.equal(getattr(lab.grades, k).view(torch.int32), getattr(gr, k).view(torch.int32)), k
    dump = lab.dump(0)
    assert sorted(dump) == ["antipodal_score", "cloud", "frame", "inv_antipodal_score", "inv_frame", "inv_search_score",
                            "normal", "search_score"]
    n = len(fx["points"])
    assert dump["cloud"].shape == (n, 3) and np.array_equal(dump["cloud"], fx["points"])
    assert dump["frame"].shape == (n, 3, 3) and dump["search_score"].shape == (n, 4, 12)
    assert dump["search_score"].dtype == np.int32 and dump["inv_antipodal_score"].dtype == np.float32
    assert (dump["search_score"] > 0).sum() > 2000
    # an unbatched cloud gets a leading 1
    one = PP.label_darboux_object(xyz[0, :, :300].contiguous(), nrm[0, :, :300].contiguous())
    assert one.unbatched and one.frames.frames.shape == (1, 300, 3, 3) and one.grades.search_score.shape == (1, 300, 2, 4, 12)


# ---- lattice clouds: every integer exact ----

def _edge_cfg(**over):
    kw = dict(theta_search_deg=(-90, 0, 90), close_region_min_points=3, back_collision_threshold=2,
              finger_collision_threshold=2)
    kw.update(over)
    return _cfg(**kw)


def _lattice(seed, n, F):
    rng = np.random.default_rng(seed)
    P, Nn = DO.lattice_cloud(rng, n)
    fr, iv = DO.axis_frames(rng, F)
    idx = rng.integers(0, n, F).astype(np.int32)
    return P, Nn, fr, iv, idx


def _edge_case(dev, seed, n, F, cfg, what, yard_frames=None):
    P, Nn, fr, iv, idx = _lattice(seed, n, F)
    got = _grade_guarded(dev, _cf(P), _cf(Nn), fr[None], iv[None], cfg, frame_index=idx[None])
    rows = np.arange(F) if yard_frames is None or yard_frames >= F else \
        np.unique(np.r_[np.arange(yard_frames // 2), np.arange(F - yard_frames // 2, F)])
    y = DO.grade64(P, Nn, fr[rows], iv[rows], cfg, index=idx[rows], eps=LATTICE_EPS)
    _check_grade({k: v[:, rows] for k, v in got.items()}, 0, y, what, exact_integers=True)
    return y


@pytest.mark.parametrize("n", [1, 4, 9, 60])
def test_tiny_clouds(dev, n):
    """N = 1, N < 5, an empty chunk (N = 9 with 8 chunks: chunk 4 holds one point, 5..7 none), and the smallest cloud
    that fills a slab."""
    y = _edge_case(dev, 10 + n, n, 2 * n, _edge_cfg(), "N=%d" % n)
    if n < 8:
        assert (y["outcome"] == 0).all()                                 # fewer than NUM_POINTS_THRESHOLD points: all slab skips
    if n == 60:
        assert (y["search_score"] > 0).any() and len(np.unique(y["outcome"])) >= 3


@pytest.mark.parametrize("n", [8191, 8192, 8193])
def test_chunk_edge(dev, n):
    """N / 8 at the sweep width (1 024 points per chunk, one full sweep), one below, and one above, where the chunk
    count turns from 8 to 9."""
    assert (n + DO.CHUNK_POINTS - 1) // DO.CHUNK_POINTS == (8 if n <= 8192 else 9)
    _edge_case(dev, n, n, 6, _edge_cfg(close_region_min_points=10, back_collision_threshold=1e4,
                                       finger_collision_threshold=1e4), "N=%d" % n)


def test_more_than_one_sweep_per_chunk(dev):
    """64 chunks at most: from N = 65 537 on a chunk holds more than one sweep of 1 024 points."""
    n = 64 * DO.SWEEP + 64 * 3 + 1
    y = _edge_case(dev, 3, n, 4, _edge_cfg(close_region_min_points=10, back_collision_threshold=1e5,
                                           finger_collision_threshold=1e5), "N=%d" % n)
    assert (y["search_score"] > 0).any()


@pytest.mark.parametrize("F", [63, 64, 65, 511, 512, 513])
def test_frame_edges(dev, F):
    """Rows are frames x 2: the grid width (128 rows = 64 frames) and the pass (1 024 rows = 512 frames) +- one frame."""
    assert DO.GRID_X == 128 and DO.PASS_ROWS == 1024
    y = _edge_case(dev, 100 + F, 150, F, _edge_cfg(), "F=%d" % F, yard_frames=24)
    assert (y["search_score"] > 0).any()


def test_lists_at_the_compiled_maxima(dev):
    """8 depths x 16 rolls x 4 shifts: fewer rows fit a pass (the LDS tables of a row are 16 KB then)."""
    cfg = _edge_cfg(length_search=tuple(-0.08 + 0.01 * i for i in range(8)),
                    theta_search_deg=tuple([-90, 0, 90, 180] * 4), shift_search=(-0.02, 0.02, 0.01, 0))
    y = _edge_case(dev, 77, 120, 40, cfg, "maxima", yard_frames=8)
    assert (y["search_score"] > 0).any()
    from s4g_release_amd import postprocess as PP
    with pytest.raises(ValueError):
        PP.DarbouxObjectConfig(shift_search=(0,) * 5).check()


def test_batch_count_nan_and_padding(dev):
    """B = 3 with unequal count; a NaN point in one object changes no other object and no other row's integers beyond
    dropping out of the counts; padding rows fail and read zero; every object equals itself alone."""
    cfg = _edge_cfg()
    sizes = [150, 37, 90]
    N = 150
    xyz = np.zeros((3, 3, N), np.float32)
    nrm = np.zeros((3, 3, N), np.float32)
    frames = np.zeros((3, N, 3, 3), np.float32)
    inv = np.zeros((3, N, 3, 3), np.float32)
    parts = []
    for b, n in enumerate(sizes):
        P, Nn, fr, iv, _ = _lattice(200 + b, n, n)
        if b == 2:
            P[5, 1] = np.nan
        parts.append((P, Nn, fr, iv))
        xyz[b, :, :n], nrm[b, :, :n], frames[b, :n], inv[b, :n] = P.T, Nn.T, fr, iv
        xyz[b, :, n:] = 1e30                                             # never read as points
        frames[b, n:], inv[b, n:] = np.eye(3), np.eye(3)                 # frames of padding rows: fail all the same
    both = _grade_guarded(dev, xyz, nrm, frames, inv, cfg, count=sizes)
    for b, (n, (P, Nn, fr, iv)) in enumerate(zip(sizes, parts)):
        y = DO.grade64(P, Nn, fr, iv, cfg, eps=LATTICE_EPS)
        got = {k: v[:, :n] for k, v in both.items()}
        _check_grade(got, b, y, "batch %d" % b, exact_integers=True)
        assert (both["fail"][b, n:] == 1).all() and not both["search"][b, n:].any() and not both["counts"][b, n:].any()
        assert not both["antipodal"][b, n:].any() and not both["slab"][b, n:].any()
        alone = _grade_guarded(dev, _cf(P), _cf(Nn), fr[None], iv[None], cfg)
        for k in both:
            assert np.array_equal(both[k][b, :n].view(np.int32), alone[k][0].view(np.int32)), (b, k)
        if b == 2:
            assert y["fail"][5].all() and not y["fail"][:5].any()        # the NaN point's own frames fail, no other
    # without the NaN the other rows of object 2 count one point more somewhere, and objects 0 and 1 do not move
    P, Nn, fr, iv = parts[2]
    healed = P.copy()
    healed[5, 1] = 0.0
    xyz2 = xyz.copy()
    xyz2[2, :, :90] = healed.T
    again = _grade_guarded(dev, xyz2, nrm, frames, inv, cfg, count=sizes)
    for k in both:
        assert np.array_equal(both[k][:2].view(np.int32), again[k][:2].view(np.int32)), k


def test_frames_edges_count_and_nan(dev):
    """The frame kernel: N < 5 (zero frames, flag 4), count shorter than N, a NaN point, batch invariance."""
    fx = _fixture()
    # a dense patch: the 700 points nearest to point 0, in their order of the cloud (the first 500 of them, too, are
    # then mostly near each other)
    patch = np.sort(np.argsort(np.linalg.norm(fx["points"] - fx["points"][0], axis=1), kind="stable")[:700])
    P, Nn = fx["points"][patch].copy(), fx["normals"][patch].copy()
    few = _frames_guarded(dev, _cf(P[:4]), _cf(Nn[:4]))
    assert (few["flags"][0] == 4).all() and not few["frames"].any() and not few["inv_frames"].any()
    one = _frames_guarded(dev, _cf(P[:1]), _cf(Nn[:1]))
    assert one["neighbours"][0, 0] == 1 and one["flags"][0, 0] == 4
    alone = _frames_guarded(dev, _cf(P[:500]), _cf(Nn[:500]))
    y = DO.frames64(P[:500], Nn[:500])
    sure = ~y["near"]
    assert np.array_equal(alone["neighbours"][0][sure], y["count"][sure])
    assert np.array_equal(alone["flags"][0][sure & (y["flags"] != 1)], y["flags"][sure & (y["flags"] != 1)])
    ok = DO.frames_decided(y)
    assert ok.sum() >= 50
    err = DO.flip_distance(alone["frames"][0], y["frames"])
    assert (err[ok] <= FRAME_FACTOR * float(fx["margin"][0]) / y["gap"][ok]).all()
    # in a batch, padded to 700 with another object's points behind the count: the same bits
    xyz = np.stack([P.T, P.T, P.T])
    nrm = np.stack([Nn.T, Nn.T, Nn.T])
    xyz[2, 0, 17] = np.nan
    from s4g_release_amd import postprocess as PP
    cnt = torch.tensor([700, 500, 700], dtype=torch.int64, device=dev)
    d = PP.estimate_object_frames(_t(xyz, dev), _t(nrm, dev), cnt)
    for k in ("frames", "inv_frames", "neighbours", "flags"):
        a = getattr(d, k)[1, :500].cpu().numpy()
        assert np.array_equal(a.view(np.int32), alone[k][0].view(np.int32)), k
        assert not getattr(d, k)[1, 500:].any(), k
    whole = _frames_guarded(dev, _cf(P), _cf(Nn))
    assert np.array_equal(d.frames[0].cpu().numpy().view(np.int32), whole["frames"][0].view(np.int32))
    # the NaN point: its own row degenerate, its neighbours' counts one short, rows away from it as without it
    assert int(d.flags[2, 17]) == 2 and not d.frames[2, 17].any()
    far = np.linalg.norm(P - P[17], axis=1) > 0.011
    assert np.array_equal(d.neighbours[2].cpu().numpy()[far], whole["neighbours"][0][far])


def test_run_to_run_graph_and_no_sync(dev):
    from s4g_release_amd import postprocess as PP
    fx = _fixture()
    xyz = _t(_cf(fx["points"][:1500]), dev)
    nrm = _t(_cf(fx["normals"][:1500]), dev)
    bits = lambda o: [t.view(torch.int32) for t in (o.frames.frames, o.frames.inv_frames, o.frames.neighbours,   # noqa: E731
                                                    o.frames.flags, o.grades.search_score, o.grades.antipodal_score,
                                                    o.grades.counts, o.grades.slab_count, o.grades.fail_i32)]
    eager = PP.label_darboux_object(xyz, nrm)
    again = PP.label_darboux_object(xyz, nrm)
    assert all(torch.equal(a, b) for a, b in zip(bits(eager), bits(again)))
    assert (eager.grades.search_score > 0).any()
    torch.cuda.synchronize(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        PP.label_darboux_object(xyz, nrm)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    run = lambda: PP.label_darboux_object(xyz, nrm)                      # noqa: E731
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for t in bits(out):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert all(torch.equal(a, b) for a, b in zip(bits(eager), bits(out)))


def test_refusals(dev):
    from s4g_release_amd import _cabi, postprocess as PP
    P, Nn, fr, iv, idx = _lattice(1, 20, 20)
    xyz, nrm = _t(_cf(P), dev), _t(_cf(Nn), dev)
    with pytest.raises(RuntimeError, match="frames must be"):
        PP.grade_object_frames(xyz, nrm, _t(fr[None, :5], dev), _t(iv[None, :5], dev))
    with pytest.raises(RuntimeError, match="int32"):
        PP.grade_object_frames(xyz, nrm, _t(fr[None], dev), _t(iv[None], dev), frame_index=_t(idx[None], dev).long())
    with pytest.raises(ValueError):
        PP.grade_object_frames(xyz, nrm, _t(fr[None], dev), _t(iv[None], dev), config=_cfg(shift_search=(0,) * 5))
    # beyond the frame kernel's limit on N: an error code, nothing launched
    big = torch.zeros((1, 3, 65537), device=dev)
    with pytest.raises(ValueError, match="65536"):
        PP.estimate_object_frames(big, big)
    out = torch.zeros((65537 * 9,), device=dev)
    rc = _cabi.lib().s4g_darboux_object_frames_f32(big.data_ptr(), big.data_ptr(), None, 1, 65537, 0.01, 5,
                                                   out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                                   out.data_ptr(), 1 << 20, None)
    assert rc == _cabi.S4G_EINVAL
    # an out-of-range frame index fails its row and nothing else
    bad = idx.copy()
    bad[3], bad[7] = -1, 20
    got = _grade_guarded(dev, _cf(P), _cf(Nn), fr[None], iv[None], _edge_cfg(), frame_index=bad[None])
    assert (got["fail"][0, [3, 7]] == 1).all() and got["fail"][0].sum() == 4
    # a zero frame fails (decision 2), its opposite direction with a real frame does not
    fz = fr.copy()
    fz[2] = 0
    got = _grade_guarded(dev, _cf(P), _cf(Nn), fz[None], iv[None], _edge_cfg(), frame_index=idx[None])
    assert got["fail"][0, 2].tolist() == [1, 0] and got["fail"][0].sum() == 1


def test_compose_scene(dev):
    from s4g_release_amd import postprocess as PP
    P0, N0, _, _, _ = _lattice(31, 80, 1)
    P1, N1, _, _, _ = _lattice(32, 50, 1)
    xyz = np.zeros((2, 3, 80), np.float32)
    nrm = np.zeros((2, 3, 80), np.float32)
    xyz[0], nrm[0] = P0.T, N0.T
    xyz[1, :, :50], nrm[1, :, :50] = P1.T, N1.T
    cnt = torch.tensor([80, 50], dtype=torch.int64, device=dev)
    obj = PP.label_darboux_object(_t(xyz, dev), _t(nrm, dev), config=_edge_cfg(), count=cnt)
    poses = [(0.1, -0.2, 0.8, 0.9238795, 0.0, 0.0, 0.3826834), (-0.05, 0.1, 0.78, 0.5, 0.5, 0.5, 0.5)]
    scene = PP.compose_darboux_scene([(obj, 0), (obj, 1)], poses, labels=[7, 3])
    dump = scene.dump()
    assert sorted(dump) == ["antipodal_score", "cloud", "frame", "inv_antipodal_score", "inv_frame", "inv_search_score",
                            "label", "normal", "search_score"]
    # data_scene_generator.py:59-103 in numpy
    clouds, normals, frames, invs, labels, ss, iss, aa, ia = [], [], [], [], [], [], [], [], []
    for b, (n, pose, lab) in enumerate(zip((80, 50), poses, (7, 3))):
        m = PP.pose_matrix(pose).numpy()
        rot = m[:3, :3]
        pc = xyz[b, :, :n].T.astype(np.float64)
        clouds.append((m @ np.concatenate([pc, np.ones((n, 1))], 1).T)[:3].T)
        normals.append((rot @ nrm[b, :, :n].astype(np.float64)).T)
        frames.append(np.matmul(rot, obj.frames.frames[b, :n].cpu().numpy().astype(np.float64)))
        invs.append(np.matmul(rot, obj.frames.inv_frames[b, :n].cpu().numpy().astype(np.float64)))
        labels.append(np.ones(n) * lab)
        ss.append(obj.grades.search_score[b, :n, 0].cpu().numpy())
        iss.append(obj.grades.search_score[b, :n, 1].cpu().numpy())
        aa.append(obj.grades.antipodal_score[b, :n, 0].cpu().numpy())
        ia.append(obj.grades.antipodal_score[b, :n, 1].cpu().numpy())
    # fp32 against float64: the pose rounded to fp32 (three entries of a row, 2^-24 each, times coordinates below 1) and
    # six roundings of partial sums below 1: 9 * 2^-24 = 5.4e-7
    tol = 9 * 2.0 ** -24
    assert dump["cloud"].shape == (130, 3) and np.abs(dump["cloud"] - np.concatenate(clouds)).max() <= tol
    assert np.abs(dump["normal"] - np.concatenate(normals)).max() <= tol
    assert np.abs(dump["frame"] - np.concatenate(frames)).max() <= tol
    assert np.abs(dump["inv_frame"] - np.concatenate(invs)).max() <= tol
    assert np.array_equal(dump["label"], np.concatenate(labels))
    assert np.array_equal(dump["search_score"], np.concatenate(ss))
    assert np.array_equal(dump["inv_search_score"], np.concatenate(iss))
    assert np.array_equal(dump["antipodal_score"].view(np.int32), np.concatenate(aa).view(np.int32))
    assert np.array_equal(dump["inv_antipodal_score"].view(np.int32), np.concatenate(ia).view(np.int32))
    assert dump["search_score"].shape == (130, 4, 3)
