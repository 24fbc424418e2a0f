"""The normal estimation on the device (`postprocess.estimate_normals`, csrc/match_normals.hip; the reference's
`PointCloud.estimate_normals`, data_gen/pcd_classes/pointcloud.py:48-60) against the fixture of tests/golden/normals.npz
and the float64 yardstick of tests/normals_ref.py (checked on the CPU by tests/test_normals_ref.py).

Tolerance, per row with count >= 3: sin(angle to the float64 normal) <= 8 * margin / g, g = (l1 - l0) / l2 the relative
gap of the float64 covariance and `margin` the fixture case's largest (distance of the yardstick's fp32 restatement from
float64) * g.  The factor 8 is tests/test_darboux_gpu.py's, for the same reason: another summation order and another
solver, each worth a few ulps of l2.  The sign must match wherever |n64 . (camera - p)| / |camera - p| > 1e-6; elsewhere
the comparison is modulo the sign.  Counts and flags are exact on every row: the neighbour set is the pinned fp32 one.
The constructions outside the fixture take their margin from the same restatement on their own input, plus 2^-23 for
the rounding of the output to fp32 (on exact inputs the restatement's own distance can be 0)."""
import numpy as np
import pytest
import torch

from tests import golden_util as GU
from tests import match_normals_ref as MR
from tests import normals_ref as NR

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -559038737
R = 0.01
H = R * (1 + 1 / 256)          # the grid's cell edge
ROUND = 2.0 ** -23


def _t(a, dev):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _guarded(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _abi(dev, cloud, camera=None, live=None, radius=R, max_nn=30, expect=0):
    """s4g_estimate_normals_f32 through the C ABI, every output in a sentinel-filled buffer with guard words and the
    workspace between guard bytes.  cloud (B, 3, N), camera (B, 3) or None, live (B,) or None -> (normals (B, 3, N)
    fp32, count (B, N), flags (B, N)) as numpy arrays."""
    from s4g_release_amd import _cabi
    from s4g_release_amd import functions as Fn
    L = _cabi.lib()
    xyz = _t(np.asarray(cloud, np.float32), dev)
    B, _, N = xyz.shape
    cam = None if camera is None else _t(np.asarray(camera, np.float32).reshape(B, 3), dev)
    lv = None if live is None else _t(np.asarray(live, np.int32), dev)
    shapes = dict(normals=(B, 3, N), count=(B, N), flags=(B, N))
    bufs = {k: _guarded(s, dev) for k, s in shapes.items()}
    nbytes = int(L.s4g_estimate_normals_workspace_bytes(B, N))
    ws = torch.full((nbytes + 2 * GUARD * 4,), 0x5A, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.s4g_estimate_normals_f32(xyz.data_ptr(), None if cam is None else cam.data_ptr(),
                                        None if lv is None else lv.data_ptr(), B, N, float(radius), int(max_nn),
                                        bufs["normals"][1].data_ptr(), bufs["count"][1].data_ptr(),
                                        bufs["flags"][1].data_ptr(), ws[GUARD * 4:].data_ptr(), nbytes, Fn._stream())
    torch.cuda.synchronize(dev)
    assert rc == expect, rc
    for k, (buf, _) in bufs.items():
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "guard of %s" % k
    assert (ws[:GUARD * 4] == 0x5A).all() and (ws[GUARD * 4 + nbytes:] == 0x5A).all(), "guard of the workspace"
    if expect != 0:
        for k, (buf, _) in bufs.items():
            assert (buf == SENTINEL).all(), k
        return None
    for k, (_, view) in bufs.items():
        assert (view != SENTINEL).all(), "%s was not written everywhere" % k
    return (bufs["normals"][1].view(torch.float32).view(B, 3, N).cpu().numpy(),
            bufs["count"][1].view(B, N).cpu().numpy(), bufs["flags"][1].view(B, N).cpu().numpy())


def _check(res, b, cloud, camera, what, radius=R, max_nn=30, live=None, margin=None, y=None):
    """Scene b of `res` against the yardstick: count and flags exact on EVERY row, the normals within the bound (and
    exact where no plane is fitted).  margin=None: the case's own restatement margin plus the output's rounding."""
    normals, count, flags = res
    if y is None:
        y = NR.normals_ref(cloud, camera, radius, max_nn, live=live)
    got = normals[b].T.astype(np.float64)
    assert np.array_equal(count[b], y["count"]), what
    assert np.array_equal(flags[b], y["flags"]), what
    plane = (y["count"] >= NR.FEW_BELOW) & ((y["flags"] & (NR.DEGENERATE | NR.PADDING | NR.NONFINITE)) == 0)
    assert np.array_equal(got[~plane], y["normals"][~plane]), what            # (0, 0, +-1) and zero rows: exactly
    extra = 0.0
    if margin is None:
        y32 = NR.normals_ref(cloud, camera, radius, max_nn, live=live, dtype=np.float32)
        use = plane & (y["gap"] > 0)
        margin = float((NR.row_error(y32["normals"], y) * y["gap"])[use].max(initial=0.0))
        extra = ROUND
    assert np.abs(np.linalg.norm(got[plane], axis=1) - 1).max(initial=0.0) < 1e-6, what
    err = NR.row_error(got, y)
    bound = NR.bound(y, margin) + extra
    judged = plane & (y["gap"] >= 1e-3)
    worst = float((err / bound)[judged].max(initial=0.0))
    print("%s: %d rows, %d judged, count %d..%d, worst err / bound = %.3g (margin %.3g)"
          % (what, len(plane), int(judged.sum()), int(y["count"].min()), int(y["count"].max()), worst, margin))
    assert (err[judged] <= bound[judged]).all(), (what, worst)
    return y


def _same(a, b):
    return all(np.array_equal(x.view(np.int32), z.view(np.int32)) for x, z in zip(a, b))


def _cluster(rng, n, spread, centre=(0.0, 0.0, 0.0)):
    """n points of a gently curved patch inside a box of edge `spread` about centre -> (3, n) fp32."""
    ab = rng.uniform(-0.5, 0.5, (n, 2)) * spread
    z = 0.3 * ab[:, 0] - 0.2 * ab[:, 1] + 4.0 * ab[:, 0] * ab[:, 1] + rng.normal(0, 0.02 * spread, n)
    return (np.asarray(centre) + np.stack([ab[:, 0], ab[:, 1], z], 1)).astype(np.float32).T.copy()


CAM = np.array([0.2, -0.1, 1.0], np.float32)


# ---- the fixture --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("r10", "r15", "lattice", "sphere"))
def test_fixture(dev, name):
    from s4g_release_amd import postprocess as PP
    fx = GU.load("normals.npz")
    pre = name + "/" if name in ("lattice", "sphere") else ""
    cloud, camera = fx[pre + "cloud"], fx[pre + "camera"]
    radius, max_nn, margin = float(fx[name + "/radius"][0]), int(fx[name + "/max_nn"][0]), float(fx[name + "/margin"][0])
    y = {k: fx["%s/%s" % (name, k)] for k in ("normals", "count", "flags", "gap", "towards")}
    res = _abi(dev, cloud[None], camera[None], None, radius, max_nn)
    _check(res, 0, cloud, camera, "fixture " + name, radius, max_nn, margin=margin, y=y)
    # every row's sign faces the camera, and the Python layer gives the same bits
    assert ((res[0][0].T.astype(np.float64) * (camera.astype(np.float64) - cloud.T.astype(np.float64))).sum(1) >= 0).all()
    e = PP.estimate_normals(_t(cloud, dev), _t(camera, dev), radius, max_nn)
    assert e.unbatched and _same((e.normals.cpu().numpy(), e.count.cpu().numpy(), e.flags.cpu().numpy()), res)
    assert np.array_equal(e.capped[0].cpu().numpy(), (y["flags"] & NR.CAPPED) != 0)
    assert np.array_equal(e.few[0].cpu().numpy(), y["count"] < 3) and not e.padding.any() and not e.nonfinite.any()


# ---- sizes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", (1, 2, 3, 4, 5, 63, 64, 65))
def test_cloud_sizes(dev, N):
    """The `few` boundary (1, 2, 3), the queries of one workgroup (4, 5), one candidate batch (63, 64, 65)."""
    cloud = _cluster(np.random.RandomState(N), N, 0.8 * R)
    res = _abi(dev, cloud[None], CAM[None])
    y = _check(res, 0, cloud, CAM, "N = %d" % N)
    assert (y["count"] == min(N, 30)).all()
    if N < 3:
        assert (res[2] == NR.FEW).all() and (res[0][0].T == [0, 0, 1]).all()


@pytest.mark.parametrize("k,max_nn", ((29, 30), (30, 30), (31, 30), (127, 30), (128, 30), (129, 30), (200, 30), (100, 1),
                                      (100, 3), (100, 64), (63, 64), (64, 64), (65, 64), (2, 3), (3, 3), (4, 3)))
def test_neighbourhood_sizes(dev, k, max_nn):
    """k points inside everyone's radius: max_nn - 1, max_nn, max_nn + 1; the cuts of the 128-key list (127, 128, 129,
    200); every max_nn of {1, 3, 30, 64}."""
    cloud = _cluster(np.random.RandomState(k + max_nn), k, 0.5 * R)
    res = _abi(dev, cloud[None], CAM[None], max_nn=max_nn)
    y = _check(res, 0, cloud, CAM, "k = %d, max_nn = %d" % (k, max_nn), max_nn=max_nn)
    assert (y["inside"] == k).all() and (y["count"] == min(k, max_nn)).all()
    assert (((res[2][0] & NR.CAPPED) != 0) == (k > max_nn)).all()


def test_lattice_ties_at_the_cap(dev):
    """Every distance on the sheet is tied many times over; the normals tell which of the tied points were kept (the
    yardstick with the tie rule reversed misses by far more than the bound, tests/test_normals_ref.py)."""
    sheet = NR.lattice_sheet(side=12, seed=3)
    cam = np.array([0.1, 0.2, 1.0], np.float32)
    for max_nn in (5, 13, 30):
        res = _abi(dev, sheet[None], cam[None], radius=5.0 / 64, max_nn=max_nn)
        y = _check(res, 0, sheet, cam, "lattice sheet, max_nn = %d" % max_nn, 5.0 / 64, max_nn)
        assert ((y["flags"] & NR.CAPPED) != 0).sum() >= 100                # (a corner of the sheet holds 22 points)
        rev = NR.normals_ref(sheet, cam, 5.0 / 64, max_nn, variant="tie reversed")
        assert (NR.row_error(rev["normals"], y) > 1e-3).sum() >= 20


def test_duplicated_points(dev):
    """A cloud drawn with replacement: queries with copies at lower and at higher indices, and neighbourhoods of
    nothing but copies, which are degenerate (and few where there are fewer than three)."""
    rng = np.random.RandomState(5)
    base = _cluster(rng, 40, 1.5 * R)
    far = np.array([[1.0], [1.0], [1.0]], np.float32)
    cloud = np.concatenate([base[:, :10], base, far, far, far, far, base[:, 30:], far + 1, far + 1], 1)
    res = _abi(dev, cloud[None], CAM[None], max_nn=30)
    y = _check(res, 0, cloud, CAM, "duplicates")
    four, two = np.arange(50, 54), np.arange(64, 66)
    assert (res[2][0][four] == NR.DEGENERATE).all() and (res[1][0][four] == 4).all()
    assert (res[2][0][two] == NR.FEW).all() and (np.abs(res[0][0].T[np.concatenate([four, two])]) == [0, 0, 1]).all()
    # max_nn = 3 on the four copies: every query keeps the three lowest indices, the last one not even itself
    res = _abi(dev, cloud[None], None, max_nn=3)
    _check(res, 0, cloud, None, "duplicates, max_nn = 3", max_nn=3)
    assert (res[2][0][four] == (NR.DEGENERATE | NR.CAPPED)).all()


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_axis_aligned_lattice_planes_are_exact(dev, axis):
    side = 9
    a, b = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    pts = np.zeros((3, side * side))
    pts[(axis + 1) % 3], pts[(axis + 2) % 3] = a.ravel() / 64, b.ravel() / 64
    pts[axis] = 0.25
    pts = pts.astype(np.float32)
    e = np.zeros(3, np.float32)
    e[axis] = 1
    for sign in (1.0, -1.0):
        cam = np.full(3, 0.05, np.float32)
        cam[axis] = 0.25 + sign
        n, c, f = _abi(dev, pts[None], cam[None], radius=3.5 / 64)
        assert np.array_equal(n[0].T.view(np.int32), np.tile(sign * e, (side * side, 1)).astype(np.float32).view(np.int32))
        assert (c[0] >= 9).all() and ((f[0] & ~NR.CAPPED) == 0).all()
    in_plane = np.full(3, 0.05, np.float32)
    in_plane[axis] = 0.25                                                  # n . (camera - p) is exactly 0: the leading sign
    for cam in (None, in_plane[None], np.full((1, 3), np.inf, np.float32), np.full((1, 3), np.nan, np.float32)):
        n, _, _ = _abi(dev, pts[None], cam, radius=3.5 / 64)
        assert np.array_equal(n[0].T, np.tile(e, (side * side, 1)))


# ---- the grid's edges ---------------------------------------------------------------------------------------------

def test_toroidal_alias_and_wrap_row(dev):
    """Two clusters 64 cell edges apart fall into the same cells and must not see each other; a cluster that straddles
    the wrap of the x cells (63 | 0) and of the y and z cells is searched through two runs per row."""
    rng = np.random.RandomState(8)
    a = _cluster(rng, 150, 3 * R)
    b = _cluster(rng, 150, 3 * R, centre=(64 * H, 0, 0))
    c = _cluster(rng, 200, 4 * R, centre=(-0.2 * H, 64 * H, -128 * H))
    cloud = np.concatenate([a, b, c], 1)[:, rng.permutation(500)]
    res = _abi(dev, cloud[None], CAM[None])
    y = _check(res, 0, cloud, CAM, "alias and wrap")
    assert ((y["flags"] & NR.CAPPED) != 0).any() and (y["count"] >= 3).sum() > 400


def test_a_far_point_forces_the_scan_and_changes_no_bit(dev):
    rng = np.random.RandomState(9)
    cloud = _cluster(rng, 300, 4 * R)
    res = _abi(dev, cloud[None], CAM[None])
    _check(res, 0, cloud, CAM, "grid")
    far = np.concatenate([cloud, np.array([[5000 * R], [0], [0]], np.float32)], 1)   # outside the exactness range
    res_far = _abi(dev, far[None], CAM[None])
    assert _same([r[..., :300] for r in res_far], res)
    assert res_far[1][0, 300] == 1 and res_far[2][0, 300] == NR.FEW


# ---- points that are not finite -----------------------------------------------------------------------------------

def test_points_that_are_not_finite(dev):
    """NaN at index 0 (the grid's origin is the first live FINITE point) and inf elsewhere: they are flagged, and every
    other row equals the cloud with those points removed, bit for bit."""
    rng = np.random.RandomState(10)
    clean = _cluster(rng, 303, 4 * R)
    bad_at = np.array([0, 1, 57, 150, 307])
    cloud = np.zeros((3, 308), np.float32)
    keep = np.ones(308, bool)
    keep[bad_at] = False
    cloud[:, keep] = clean
    cloud[:, 0] = np.nan
    cloud[:, 1] = (0.0, np.inf, 0.0)
    cloud[:, 57] = (np.nan, 0.0, 0.0)
    cloud[:, 150] = (0.0, 0.0, -np.inf)
    cloud[:, 307] = np.inf
    res = _abi(dev, cloud[None], CAM[None])
    ref = _abi(dev, clean[None], CAM[None])
    _check(ref, 0, clean, CAM, "clean")
    assert _same([r[..., keep] for r in res], ref)
    assert (res[2][0][bad_at] == NR.NONFINITE).all() and (res[1][0][bad_at] == 0).all()
    assert (res[0][0].T[bad_at] == [0, 0, 1]).all()
    _check(res, 0, cloud, CAM, "with points that are not finite")
    # nothing finite at all
    n, c, f = _abi(dev, np.full((1, 3, 70), np.nan, np.float32), CAM[None])
    assert (f == NR.NONFINITE).all() and (c == 0).all() and (n[0].T == [0, 0, 1]).all()


# ---- the camera ---------------------------------------------------------------------------------------------------

def test_camera_cases(dev):
    rng = np.random.RandomState(11)
    cloud = _cluster(rng, 200, 3 * R)
    none = _abi(dev, cloud[None], None)
    y = _check(none, 0, cloud, None, "no camera")
    n = none[0][0].T
    lead = n[np.arange(200), np.abs(n).argmax(1)]
    assert (lead > 0).all()                                               # the leading component is positive
    for cam in (np.full(3, np.inf, np.float32), np.array([0, np.nan, 0], np.float32)):
        assert _same(_abi(dev, cloud[None], cam[None]), none)             # no direction: the same rule
    at = cloud[:, 17].copy()                                              # the camera at a query point: that row has no direction
    res = _abi(dev, cloud[None], at[None])
    _check(res, 0, cloud, at, "camera at a query")
    assert np.array_equal(res[0][0][:, 17], none[0][0][:, 17])
    below = _abi(dev, cloud[None], np.array([[0, 0, -1.0]], np.float32))
    above = _abi(dev, cloud[None], np.array([[0, 0, 1.0]], np.float32))
    assert np.array_equal(below[0], -above[0]) and np.array_equal(below[1], above[1])
    assert y["count"].min() >= 3


# ---- batches ------------------------------------------------------------------------------------------------------

def test_batches_counts_and_determinism(dev):
    """B = 1, 2, 3 with `live` of 0, 1, 2, N and above N: each scene equals its single-scene run, two runs are equal,
    padding rows are zero with their flag."""
    rng = np.random.RandomState(12)
    N = 120
    clouds = np.stack([_cluster(rng, N, 3 * R) for _ in range(3)])
    cams = np.stack([CAM, -CAM, CAM * 2])
    for lives in ((N,), (0, N + 7), (1, 2, 77), (-3, N, 2)):
        B = len(lives)
        res = _abi(dev, clouds[:B], cams[:B], lives)
        assert _same(res, _abi(dev, clouds[:B], cams[:B], lives))
        for b in range(B):
            alone = _abi(dev, clouds[b:b + 1], cams[b:b + 1], lives[b:b + 1])
            assert _same([r[b:b + 1] for r in res], alone), (lives, b)
            n_live = min(max(lives[b], 0), N)
            _check(res, b, clouds[b], cams[b], "live = %d" % lives[b], live=lives[b])
            assert (res[2][b, n_live:] == NR.PADDING).all() and (res[1][b, n_live:] == 0).all()
            assert not res[0][b][:, n_live:].any()
            # the padded rows are no keys: the live rows equal the cloud cut at live
            if 0 < n_live < N:
                cut = _abi(dev, clouds[b:b + 1, :, :n_live], cams[b:b + 1])
                assert _same([r[b:b + 1, ..., :n_live] for r in res], cut)
    full = _abi(dev, clouds, cams, None)
    assert _same(full, _abi(dev, clouds, cams, (N, N, N)))


def test_257_scenes_cross_the_chunk(dev):
    rng = np.random.RandomState(13)
    clouds = np.stack([_cluster(rng, 8, 0.5 * R) for _ in range(257)])
    cams = np.tile(CAM, (257, 1))
    res = _abi(dev, clouds, cams)
    for b in (0, 1, 255, 256):
        _check(res, b, clouds[b], CAM, "scene %d of 257" % b)
        assert _same([r[b:b + 1] for r in res], _abi(dev, clouds[b:b + 1], cams[b:b + 1]))
    assert (res[1] == 8).all() and (res[2] == 0).all()


def test_graph_replay_equals_eager(dev):
    from s4g_release_amd import postprocess as PP
    rng = np.random.RandomState(14)
    clouds = _t(np.stack([_cluster(rng, 200, 3 * R) for _ in range(2)]), dev)
    cams = _t(np.stack([CAM, -CAM]), dev)
    live = _t(np.array([200, 150], np.int32), dev)
    eager = PP.estimate_normals(clouds, cams, count=live)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        PP.estimate_normals(clouds, cams, count=live)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = PP.estimate_normals(clouds, cams, count=live)
    for t in (out.normals, out.count, out.flags):
        t.zero_()
    g.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out.normals.view(torch.int32), eager.normals.view(torch.int32))
    assert torch.equal(out.count, eager.count) and torch.equal(out.flags, eager.flags)
    assert (eager.padding[1, 150:]).all() and not eager.padding[0].any()


# ---- the Python layer ---------------------------------------------------------------------------------------------

def test_refusals(dev):
    from s4g_release_amd import postprocess as PP
    cloud = torch.zeros(1, 3, 8, device=dev)
    cam = torch.zeros(1, 3, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    for args, kw in (((cloud.cpu(),), {}), ((cloud, cam.cpu()), {}), ((cloud,), {"count": cnt.cpu()})):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            PP.estimate_normals(*args, **kw)
    for args in ((cloud.double(),), (cloud, cam.double())):
        with pytest.raises(RuntimeError, match="float32"):
            PP.estimate_normals(*args)
    with pytest.raises(RuntimeError, match=r"\(B, 3, N\)"):
        PP.estimate_normals(torch.zeros(1, 4, 8, device=dev))
    with pytest.raises(RuntimeError, match=r"\(B, 3\) or \(3,\)"):
        PP.estimate_normals(cloud, torch.zeros(2, 3, device=dev))
    with pytest.raises(RuntimeError, match="int32"):
        PP.estimate_normals(cloud, count=cnt.long())
    with pytest.raises(RuntimeError, match=r"\(B,\)"):
        PP.estimate_normals(cloud, count=torch.zeros(2, dtype=torch.int32, device=dev))
    for radius in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="radius"):
            PP.estimate_normals(cloud, radius=radius)
    for max_nn in (0, 65):
        with pytest.raises(ValueError, match="max_nn"):
            PP.estimate_normals(cloud, max_nn=max_nn)
    # the C entry refuses the same on its own, and a short workspace, and writes nothing
    z = np.zeros((1, 3, 8), np.float32)
    for radius, max_nn in ((0.0, 30), (R, 0), (R, 65), (1e19, 30), (float("nan"), 30)):
        _abi(dev, z, None, None, radius, max_nn, expect=-1)
    from s4g_release_amd import _cabi
    L = _cabi.lib()
    out = torch.full((64,), SENTINEL, dtype=torch.int32, device=dev)
    ws = torch.zeros(64, dtype=torch.uint8, device=dev)
    p = out.data_ptr()
    assert L.s4g_estimate_normals_f32(cloud.data_ptr(), None, None, 1, 8, R, 30, p, p, p, ws.data_ptr(), 64, None) == -2
    assert L.s4g_estimate_normals_f32(cloud.data_ptr(), None, None, 1, 8, R, 30, p, p, p, None, 0, None) == -2
    assert L.s4g_estimate_normals_f32(None, None, None, 1, 8, R, 30, p, p, p, ws.data_ptr(), 64, None) == -1
    assert L.s4g_estimate_normals_f32(cloud.data_ptr(), None, None, 65536, 8, R, 30, p, p, p, None, 0, None) == -1
    assert L.s4g_estimate_normals_f32(cloud.data_ptr(), None, None, 1, 1 << 30, R, 30, p, p, p, None, 0, None) == -1
    assert L.s4g_estimate_normals_f32(None, None, None, 0, 8, R, 30, None, None, None, None, 0, None) == 0
    assert L.s4g_estimate_normals_workspace_bytes(0, 8) == 0 and L.s4g_estimate_normals_workspace_bytes(1, 0) == 0
    torch.cuda.synchronize(dev)
    assert (out == SENTINEL).all()


def test_label_view_estimates_then_grades(dev):
    """`label_view(estimate_normal=True, camera=c)` equals `label_view` fed `estimate_normals(...).normals`, bit for
    bit; `estimated` is set then and None by default; it excludes `match_normal`."""
    from s4g_release_amd import postprocess as PP
    fx = GU.load("darboux.npz")
    view, scene_n, labels = _t(fx["cloud"][None], dev), _t(fx["normals"][None], dev), _t(fx["labels"][None], dev)
    cam = _t(np.array([0.5, -0.3, 1.5], np.float32), dev)
    v = PP.label_view(view, None, view, scene_n, labels, estimate_normal=True, camera=cam)
    e = PP.estimate_normals(view, cam, PP.CURVATURE_RADIUS, PP.NORMAL_MAX_NN)
    w = PP.label_view(view, e.normals, view, scene_n, labels)
    assert v.estimated is not None and w.estimated is None and v.matched is None
    assert torch.equal(v.estimated.normals.view(torch.int32), e.normals.view(torch.int32))
    assert torch.equal(v.estimated.count, e.count) and torch.equal(v.estimated.flags, e.flags)
    print("label_view(estimate_normal=True): %d valid frames, %d few rows" % (int(v.search.count[0]), int(e.few.sum())))
    for k in ("frames", "points"):
        assert torch.equal(getattr(v.darboux, k).view(torch.int32), getattr(w.darboux, k).view(torch.int32))
    assert torch.equal(v.darboux.count, w.darboux.count) and torch.equal(v.darboux.flags, w.darboux.flags)
    for k in ("ints", "slab_count", "valid_i32", "valid_index", "count"):
        assert torch.equal(getattr(v.search, k), getattr(w.search, k)), k
    assert torch.equal(v.search.scores.view(torch.int32), w.search.scores.view(torch.int32))
    assert torch.equal(v.cloud_index, w.cloud_index)
    one = PP.label_view(view[0], None, view[0], scene_n[0], labels[0], estimate_normal=True, camera=cam)
    assert one.estimated.unbatched and torch.equal(one.cloud_index, v.cloud_index)
    with pytest.raises(ValueError, match="exclude"):
        PP.label_view(view, None, view, scene_n, labels, estimate_normal=True, match_normal=True, camera=cam)


def test_label_baseline_view_estimates_missing_normals(dev):
    from s4g_release_amd import postprocess as PP
    from tests import close_region_ref as CR
    fx = CR.load_fixture()
    pts, frames, scene = _t(fx["points"], dev), _t(fx["frames"], dev), _t(fx["cloud"], dev)
    given = _t(fx["normals"], dev)
    cam = _t(np.array([0.5, -0.3, 1.5], np.float32), dev)
    est = PP.estimate_normals(scene, cam).normals[0]

    def same(a, b):
        """the reference's dump of both, array for array (the storage past a set's count is not part of it)"""
        da, db = a.dump(0), b.dump(0)
        assert sorted(da) == sorted(db) and len(da["valid_index"]) > 0
        for k in da:
            xs, ys = (v if isinstance(v, (list, tuple)) else [v] for v in (da[k], db[k]))
            assert len(xs) == len(ys), k
            for x, z in zip(xs, ys):
                x, z = np.asarray(x), np.asarray(z)
                assert x.shape == z.shape and x.tobytes() == z.tobytes(), k
        assert torch.equal(a.regions.count, b.regions.count) and torch.equal(a.best.index, b.best.index)

    # the scene without normals: estimated, then used for the search and the regions
    same(PP.label_baseline_view(pts, frames, scene, None, camera=cam), PP.label_baseline_view(pts, frames, scene, est))
    # a view cloud without normals beside a scene that has them
    same(PP.label_baseline_view(pts, frames, scene, given, cloud=scene, camera=cam),
         PP.label_baseline_view(pts, frames, scene, given, cloud=scene, normals=est))
    # given normals are used as they are, camera or not; without a camera nothing is estimated
    same(PP.label_baseline_view(pts, frames, scene, given, camera=cam), PP.label_baseline_view(pts, frames, scene, given))
    with pytest.raises(RuntimeError, match="go together"):
        PP.label_baseline_view(pts, frames, scene, given, cloud=scene)
    with pytest.raises(RuntimeError, match="go together"):
        PP.label_baseline_view(pts, frames, scene, given, normals=given, camera=cam)


def test_cloud_pre_processor_estimates_normals(dev):
    from s4g_release_amd import postprocess as PP
    from s4g_release_amd import preprocess as PRE
    fx = GU.load("normals.npz")
    cloud = _t(fx["cloud"], dev)
    cp = PRE.CloudPreProcessor(cloud)
    got = cp.estimate_normals()
    want = PP.estimate_normals(cloud, torch.zeros(3, device=dev))
    assert got is cp.normals and tuple(got.shape) == (3, cloud.shape[1])
    assert torch.equal(got.view(torch.int32), want.normals[0].view(torch.int32))
    other = PRE.CloudPreProcessor(cloud).estimate_normals(np.array([0.0, 0.0, -5.0]))
    assert not torch.equal(other, got) and torch.equal(other.abs(), got.abs())
