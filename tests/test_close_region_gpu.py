"""The baseline inputs on the device (`postprocess.best_placement`, `close_regions`, `label_baseline_view`;
csrc/close_region.hip) against the fixture the reference's own `finger_hand` and `close_region_projection` produced
(tests/golden/baseline_regions.npz) and the float64 yardstick of tests/close_region_ref.py (checked on the CPU by
tests/test_close_region_ref.py).

Tolerances.  Best index and validity exact on the fixture (its frames are decided and their best placement is clear);
score within SCORE_TOL = 1e-4, the project's bar for this score; `global_to_local` within 1e-5 of `baseline_frame`, the
bar of `frames_of`.  Sets: certain members <= returned <= certain + ambiguous (within 4e-6 of a face); coordinates
within 4e-6 of float64.  Maps against `projection64` OF THE CALL'S OWN PACKED SETS (voxel assignment is then exact):
(m + 64) * 2^-24 * s, derived in `close_region_ref.map_bound`.  Maps against the reference's: the same bound plus the
fixture's `margin`, on the frames whose index set equals the reference's, outside the pixels a point within 1e-6 of a
voxel face can move between (`close_region_ref.pixel_mask`: the reference transforms in two steps, the kernel in one, and
the two fp32 routes differ by about 1e-7); at least 90 % of the non-zero pixels must remain.

The loop-edge and capacity tests call the C ABI with every output inside a sentinel-filled buffer with guard words on
both sides, the workspace included."""
import ctypes

import numpy as np
import pytest
import torch

from s4g_release_amd.postprocess import LocalSearchConfig, ProjectionConfig
from tests import close_region_ref as CR
from tests import local_search_ref as LR

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -559038737
CFG = LocalSearchConfig()


def _t(a, dev):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _guarded(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _regions_guarded(dev, g2l, cloud, normals, live=None, frame_count=None, capacity=None, proj=None, x_range=None,
                     expect=0):
    """s4g_close_region_f32 through the C ABI, every output in a guarded buffer -> dict of numpy arrays (the float
    outputs also as their int32 bits, `*_bits`: untouched storage still holds the sentinel)."""
    from s4g_release_amd import _cabi
    from s4g_release_amd import functions as Fn
    proj = proj or ProjectionConfig()
    B, F = g2l.shape[:2]
    N = cloud.shape[2]
    R = proj.resolution
    cap = F * min(N, 4096) if capacity is None else capacity
    d_g, d_x, d_n = _t(g2l, dev), _t(cloud, dev), _t(normals, dev)
    d_l = None if live is None else _t(np.asarray(live, np.int32), dev)
    d_c = None if frame_count is None else _t(np.asarray(frame_count, np.int64), dev)
    x_lo, x_hi = (-CFG.bottom_length, CFG.finger_length) if x_range is None else x_range
    u, h = proj.units(CFG), proj.heights(CFG)
    params = (ctypes.c_float * 13)(x_lo, x_hi, CFG.half_bottom_space, CFG.half_hand_thickness, *u, *[v[0] for v in h],
                                   *[v[1] for v in h])
    shapes = dict(count=(B, F), offset=(B, F + 1, 2), points=(B, 3, cap), normals=(B, 3, cap), index=(B, cap),
                  maps=(B, F, 12, R, R), flags=(B, F))
    bufs = {k: _guarded(s, dev) for k, s in shapes.items()}
    nbytes = int(_cabi.lib().s4g_close_region_workspace_bytes(B, N, F, cap))
    ws = torch.full((nbytes + 2 * GUARD * 4,), 0x5A, dtype=torch.uint8, device=dev)
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_close_region_f32(
            d_g.data_ptr(), d_x.data_ptr(), d_n.data_ptr(), None if d_l is None else d_l.data_ptr(),
            None if d_c is None else d_c.data_ptr(), B, N, F, cap, R, params, p["count"], p["offset"], p["points"],
            p["normals"], p["index"], p["maps"], p["flags"], ws[GUARD * 4:].data_ptr(), nbytes, Fn._stream())
    assert rc == expect, rc
    torch.cuda.synchronize(dev)
    for k, (buf, _) in bufs.items():
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "guard of %s" % k
    assert (ws[:GUARD * 4] == 0x5A).all() and (ws[GUARD * 4 + nbytes:] == 0x5A).all(), "guard of the workspace"
    out = {}
    for k, (_, v) in bufs.items():
        a = v.cpu().numpy()
        if k == "offset":
            out[k] = a.view(np.int64).reshape(B, F + 1)
        elif k in ("points", "normals", "maps"):
            out[k], out[k + "_bits"] = a.view(np.float32).reshape(shapes[k]), a.reshape(shapes[k])
        else:
            out[k] = a.reshape(shapes[k])
    out["capacity"] = cap
    return out


def _check_scene(got, b, g2l, cloud, normals, live=None, frame_count=None, proj=None, x_range=None, map_frames=None):
    """Everything `close_regions` promises for scene b against the yardstick -> (stored non-empty frames, the largest
    map distance from projection64 over its bound)."""
    proj = proj or ProjectionConfig()
    F = len(g2l)
    cap = got["capacity"]
    alive = np.ones(F, bool) if live is None else np.asarray(live) != 0
    if frame_count is not None:
        alive &= np.arange(F) < frame_count
    reg = CR.regions64(g2l, cloud, CFG, x_range)
    cnt, off, flags = got["count"][b], got["offset"][b], got["flags"][b]
    assert off[0] == 0 and np.array_equal(np.diff(off), cnt)
    assert (cnt[~alive] == 0).all() and (flags[~alive] == 0).all() and not got["maps_bits"][b][~alive].any()
    fits = off[1:] <= cap
    assert np.array_equal((flags & 1) != 0, alive & ~fits)
    stored, worst, end = 0, 0.0, 0
    for f in np.nonzero(alive)[0]:
        r = reg[f]
        n_c, n_a = len(r["certain"]), len(r["ambiguous"])
        assert n_c <= cnt[f] <= n_c + n_a, (f, n_c, cnt[f], n_a)
        if flags[f]:
            assert not got["maps_bits"][b, f].any()
            continue
        lo, hi = int(off[f]), int(off[f + 1])
        end = max(end, hi)
        idx = got["index"][b, lo:hi]
        assert (np.diff(idx) > 0).all() and set(r["certain"]) <= set(idx) <= set(r["certain"]) | set(r["ambiguous"])
        if hi == lo:
            assert not got["maps_bits"][b, f].any()
            continue
        stored += 1
        p32, n32 = got["points"][b, :, lo:hi], got["normals"][b, :, lo:hi]
        assert np.abs(p32 - r["local"][:, idx]).max() < CR.TOL
        want_n = np.asarray(g2l[f], np.float64)[:3, :3] @ np.asarray(normals, np.float64)[:, idx]
        assert np.abs(n32 - want_n).max() < 1e-6 * max(1.0, float(np.abs(want_n).max()))
        if map_frames is not None and f not in map_frames:
            continue
        want, _ = CR.projection64(p32, n32, proj, CFG)
        d = np.abs(got["maps"][b, f] - want) / CR.map_bound(p32, n32, proj, CFG)
        assert d.max() <= 1.0, (f, float(d.max()))
        worst = max(worst, float(d.max()))
    for k in ("points_bits", "normals_bits"):             # storage past the last stored frame is left untouched
        assert (got[k][b][:, end:] == SENTINEL).all(), k
    assert (got["index"][b][end:] == SENTINEL).all()
    return stored, worst


# ------------------------------------------------------------------------------------------------- the reference's fixture
@pytest.fixture(scope="module")
def fx():
    return CR.load_fixture()


@pytest.fixture(scope="module")
def labels_of_fixture(fx, dev):
    from s4g_release_amd import postprocess as PP
    out = PP.label_baseline_view(_t(fx["points"], dev), _t(fx["frames"], dev), _t(fx["cloud"], dev),
                                 _t(fx["normals"], dev))
    torch.cuda.synchronize(dev)
    return out


def test_fixture_best_placement(fx, labels_of_fixture):
    best = labels_of_fixture.best
    assert best.unbatched and best.index.shape == (1, len(fx["points"]))
    idx, score, G = best.index[0].cpu().numpy(), best.score[0].cpu().numpy(), best.global_to_local[0].cpu().numpy()
    assert np.array_equal(idx >= 0, fx["valid"]) and np.array_equal(idx, fx["best_index"])
    assert np.abs(score - fx["score"]).max() <= LR.SCORE_TOL
    v = fx["valid"]
    print("global_to_local: largest distance from baseline_frame %.3g" % np.abs(G[v] - fx["baseline_frame"][v]).max())
    assert np.abs(G[v] - fx["baseline_frame"][v]).max() <= 1e-5 and not G[~v].any()
    n = int(best.count[0])
    assert n == v.sum() and np.array_equal(best.valid_index[0, :n].cpu().numpy(), np.nonzero(v)[0])
    assert (best.valid_index[0, n:] == -1).all()


def test_fixture_sets_and_maps(fx, labels_of_fixture):
    proj = ProjectionConfig()
    reg = labels_of_fixture.regions
    G = labels_of_fixture.best.global_to_local[0].cpu().numpy()
    cnt, off, flags = reg.count[0].cpu().numpy(), reg.offset[0].cpu().numpy(), reg.flags[0].cpu().numpy()
    assert not flags.any() and (cnt[~fx["valid"]] == 0).all() and not reg.maps[0][_t(~fx["valid"], reg.maps.device)].any()
    y = CR.regions64(G, fx["cloud"], CFG)
    P, Nn, I, M = (t[0].cpu().numpy() for t in (reg.points, reg.normals, reg.index, reg.maps))
    same, seen, total, worst, worst_own = 0, 0, 0, 0.0, 0.0
    vf = np.nonzero(fx["valid"])[0]
    for k, f in enumerate(vf):
        idx = I[off[f]:off[f + 1]]
        r = y[f]
        assert set(r["certain"]) <= set(idx) <= set(r["certain"]) | set(r["ambiguous"]) and (np.diff(idx) > 0).all()
        p32, n32 = P[:, off[f]:off[f + 1]], Nn[:, off[f]:off[f + 1]]
        assert np.abs(p32 - r["local"][:, idx]).max() < CR.TOL
        bound = CR.map_bound(p32, n32, proj, CFG)
        own, _ = CR.projection64(p32, n32, proj, CFG)
        assert (np.abs(M[f] - own) <= bound).all(), f
        worst_own = max(worst_own, float((np.abs(M[f] - own) / bound).max()))
        if not np.array_equal(idx, fx["set_index"][fx["set_offset"][k]:fx["set_offset"][k + 1]]):
            continue
        same += 1
        mask = CR.pixel_mask(r["local"][:, idx], proj, CFG)
        d = np.abs(M[f].astype(np.float64) - fx["maps"][k])
        assert (d <= bound + float(fx["margin"][0]))[~mask].all(), (f, float((d * ~mask).max()))
        worst = max(worst, float((d * ~mask).max()))
        nz = fx["maps"][k] != 0
        seen, total = seen + int((nz & ~mask).sum()), total + int(nz.sum())
    print("maps: %.3g of the bound from projection64 of the own sets; %.3g from the reference's on %d of %d frames, %d of "
          "%d non-zero pixels" % (worst_own, worst, same, len(vf), seen, total))
    assert same >= 0.75 * len(vf) and seen >= 0.9 * total
    d = labels_of_fixture.dump(0)
    assert len(d["close_region_points_set"]) == len(vf) and d["baseline_frame"].shape == (len(vf), 4, 4)
    assert d["close_region_projection_map_set"][0].shape == (12, 60, 60)
    assert np.array_equal(d["close_region_points_set"][3], P[:, off[vf[3]]:off[vf[3] + 1]])


def test_count_equals_the_search_close_count(fx, labels_of_fixture, dev):
    L, T = CFG.shape
    y = LR.search64(fx["points"], fx["frames"], fx["cloud"], fx["normals"], np.zeros(fx["cloud"].shape[1], np.int32), CFG)
    clear = y["clear"].reshape(-1, L * T)
    close = labels_of_fixture.search.close[0].reshape(-1, L * T).cpu().numpy()
    cnt = labels_of_fixture.regions.count[0].cpu().numpy()
    vf = np.nonzero(fx["valid"])[0]
    sure = [f for f in vf if clear[f, fx["best_index"][f]]]
    assert len(sure) >= 0.75 * len(vf)
    for f in sure:
        assert cnt[f] == close[f, fx["best_index"][f]], f


def test_faces_are_strict_on_the_device(dev):
    for x_range in (None, (0.0, CFG.finger_length)):
        cloud, member = CR.face_cloud(CFG, x_range)
        nrm = np.tile(np.array([[0.0], [1.0], [0.0]], np.float32), (1, cloud.shape[1]))
        got = _regions_guarded(dev, np.eye(4, dtype=np.float32)[None, None], cloud[None], nrm[None], x_range=x_range)
        assert got["count"][0, 0] == member.sum()
        assert np.array_equal(got["index"][0, :member.sum()], np.nonzero(member)[0])
        want = cloud[:, member].astype(np.float32).copy()
        want[1] += np.float32(CFG.half_bottom_space)
        want[2] += np.float32(CFG.half_hand_thickness)
        assert np.array_equal(got["points"][0, :, :member.sum()], want)


# -------------------------------------------------------------------------------------------------------------- loop edges
def _scene(seed, B, N, F, n_in=40):
    rng = np.random.default_rng(seed)
    parts = [CR.blob_frames(rng, N, F, CFG, n_in) for _ in range(B)]
    return tuple(np.stack([p[i] for p in parts]) for i in (2, 0, 1))          # g2l (B, F, 4, 4), cloud, normals (B, 3, N)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4 * CR.SWEEP_POINTS - 1, 4 * CR.SWEEP_POINTS + 1,
                               4 * CR.CHUNK_POINTS - 1, 4 * CR.CHUNK_POINTS + 1])
def test_point_loop_edges(dev, N):
    g2l, cloud, normals = _scene(N, 1, N, 5)
    got = _regions_guarded(dev, g2l, cloud, normals)
    stored, worst = _check_scene(got, 0, g2l[0], cloud[0], normals[0])
    print("N = %d: %d stored frames, maps at %.3g of the bound" % (N, stored, worst))
    assert stored >= 1


@pytest.mark.parametrize("F", [CR.FRAMES_PER_PASS - 1, CR.FRAMES_PER_PASS, CR.FRAMES_PER_PASS + 1])
def test_frame_loop_edges(dev, F):
    g2l, cloud, normals = _scene(F, 1, 300, F)
    got = _regions_guarded(dev, g2l, cloud, normals)
    stored, worst = _check_scene(got, 0, g2l[0], cloud[0], normals[0], map_frames=set(range(0, F, 23)) | {F - 2, F - 1})
    print("F = %d: %d stored frames, maps at %.3g of the bound" % (F, stored, worst))
    assert stored >= F - 2


@pytest.mark.parametrize("B", [1, 3])
def test_batches_frame_counts_and_live_masks(dev, B):
    F = 40
    g2l, cloud, normals = _scene(100 + B, B, 1500, F, n_in=300)
    counts = np.array([F, 0, 17][:B], np.int64) if B > 1 else np.array([F - 3], np.int64)
    live = (np.random.default_rng(B).random((B, F)) < 0.7).astype(np.int32)
    live[:, 0] = 1
    for use_live, use_count in ((True, True), (True, False), (False, True)):
        got = _regions_guarded(dev, g2l, cloud, normals, live if use_live else None, counts if use_count else None)
        for b in range(B):
            stored, _ = _check_scene(got, b, g2l[b], cloud[b], normals[b], live[b] if use_live else None,
                                     int(counts[b]) if use_count else None, map_frames={0, 5, 16, F - 1})
            assert stored >= 1 or (use_count and counts[b] == 0)


@pytest.mark.parametrize("R", [60, 64, 7])
def test_resolutions(dev, R):
    proj = ProjectionConfig(resolution=R)
    g2l, cloud, normals = _scene(R, 1, 2000, 6, n_in=1200)              # (dense: several points per voxel at R = 7)
    got = _regions_guarded(dev, g2l, cloud, normals, proj=proj, x_range=(0.0, CFG.finger_length))
    stored, worst = _check_scene(got, 0, g2l[0], cloud[0], normals[0], proj=proj, x_range=(0.0, CFG.finger_length))
    print("R = %d: %d stored frames, maps at %.3g of the bound" % (R, stored, worst))
    assert stored == 6


def test_capacity_edges(dev):
    g2l, cloud, normals = _scene(77, 1, 500, 9, n_in=60)
    full = _regions_guarded(dev, g2l, cloud, normals)
    total = int(full["offset"][0, -1])
    last = int(np.nonzero(full["count"][0])[0][-1])
    assert total > 0 and not full["flags"].any()
    for cap in (total, total - 1, 0):
        got = _regions_guarded(dev, g2l, cloud, normals, capacity=cap)
        assert np.array_equal(got["count"], full["count"]) and np.array_equal(got["offset"], full["offset"])
        _check_scene(got, 0, g2l[0], cloud[0], normals[0])
        flagged = np.nonzero(got["flags"][0] & 1)[0]
        if cap == total:
            assert len(flagged) == 0 and np.array_equal(got["maps_bits"], full["maps_bits"])
            assert np.array_equal(got["index"][0], full["index"][0, :total])
        elif cap == total - 1:
            assert flagged[0] == last and not got["maps_bits"][0, last].any()
            assert np.array_equal(got["maps_bits"][0, :last], full["maps_bits"][0, :last])
        else:
            assert np.array_equal(flagged, np.nonzero(full["offset"][0, 1:] > 0)[0]) and not got["maps_bits"].any()


# ------------------------------------------------------------------------------------------------ determinism and capture
FIELDS = ("count", "offset", "points", "normals", "index", "maps", "flags")


def _same(a, b, sa=None, sb=None):
    """Scene sb of b against scene sa of a (default: every scene against itself), bit for bit; the packed buffers up to
    the scene's own total (storage behind it is left untouched)."""
    if sa is None:
        return a.count.shape == b.count.shape and all(_same(a, b, s, s) for s in range(a.count.shape[0]))
    n = int(a.offset[sa, -1])
    for k in FIELDS:
        x, y = getattr(a, k)[sa], getattr(b, k)[sb]
        if k in ("points", "normals", "index"):
            x, y = x[..., :n], y[..., :n]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        if not torch.equal(x, y):
            return False
    return True


def test_runs_batches_and_graph_replays_are_bit_identical(dev):
    from s4g_release_amd import postprocess as PP
    g2l, cloud, normals = (_t(a, dev) for a in _scene(9, 3, 3000, 50, n_in=700))
    cnt = torch.tensor([50, 31, 7], device=dev)
    cap = 50 * 800
    run = lambda s=slice(None): PP.close_regions(g2l[s], cloud[s], normals[s], frame_count=cnt[s], capacity=cap)
    a, b = run(), run()
    torch.cuda.synchronize(dev)
    assert not a.flags.any() and int(a.count.sum()) > 3000
    assert _same(a, b)
    for s in range(3):
        assert _same(run(slice(s, s + 1)), a, 0, s), s
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    for _ in range(2):
        for k in FIELDS:
            getattr(out, k).zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        assert _same(out, a)


def test_a_nan_normal_flags_its_frames_only(dev):
    from s4g_release_amd import postprocess as PP
    g2l, cloud, normals = _scene(21, 2, 800, 12, n_in=100)
    clean = PP.close_regions(_t(g2l, dev), _t(cloud, dev), _t(normals, dev))
    idx0 = clean.index[0, :int(clean.offset[0, 1])].cpu().numpy()
    victim = int(idx0[len(idx0) // 2])                                   # a member of frame 0 of scene 0
    bad = normals.copy()
    bad[0, 1, victim] = np.nan
    got = PP.close_regions(_t(g2l, dev), _t(cloud, dev), _t(bad, dev))
    torch.cuda.synchronize(dev)
    holds = np.array([victim in clean.index[0, int(clean.offset[0, f]):int(clean.offset[0, f + 1])].cpu().numpy()
                      for f in range(12)])
    assert holds[0] and np.array_equal((got.flags[0].cpu().numpy() & 2) != 0, holds) and not got.flags[1].any()
    assert torch.equal(got.count, clean.count) and torch.equal(got.offset, clean.offset)
    for b in range(2):
        n = int(clean.offset[b, -1])
        assert torch.equal(got.index[b, :n], clean.index[b, :n])
        assert torch.equal(got.points[b, :, :n].view(torch.int32), clean.points[b, :, :n].view(torch.int32))
    keep = _t(~holds, dev)
    assert torch.equal(got.maps[0][keep].view(torch.int32), clean.maps[0][keep].view(torch.int32))
    assert not got.maps[0][~keep].any() and torch.equal(got.maps[1].view(torch.int32), clean.maps[1].view(torch.int32))


def test_argument_errors_come_before_any_launch(dev):
    from s4g_release_amd import postprocess as PP
    g2l, cloud, normals = _scene(3, 1, 64, 2)
    G, X, Nn = _t(g2l, dev), _t(cloud, dev), _t(normals, dev)
    for args in ((G.cpu(), X, Nn), (G, X.cpu(), Nn), (G, X, Nn.cpu())):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            PP.close_regions(*args)
    for args in ((G[:, :, :3], X, Nn), (G, X[:, :2], Nn), (G, X, Nn[:, :, :5]), (G, X.double(), Nn)):
        with pytest.raises(RuntimeError):
            PP.close_regions(*args)
    with pytest.raises(RuntimeError, match="live"):
        PP.close_regions(G, X, Nn, live=torch.ones(1, 3, device=dev))
    with pytest.raises(ValueError, match="resolution"):
        PP.close_regions(G, X, Nn, projection=ProjectionConfig(resolution=65))
    with pytest.raises(ValueError, match="capacity"):
        PP.close_regions(G, X, Nn, capacity=2 ** 31)
    with pytest.raises(RuntimeError, match="LocalSearch"):
        PP.best_placement(G)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        PP.label_baseline_view(torch.zeros(2, 3), torch.zeros(2, 3, 3), X[0].cpu(), Nn[0].cpu())
    # the C entry itself: sizes and the resolution are refused before any launch (no output is touched)
    assert _regions_guarded_raw_resolution(dev, g2l, cloud, normals, 65) == -1
    from s4g_release_amd import _cabi
    assert _cabi.lib().s4g_close_region_workspace_bytes(1, 64, 2, 2 ** 31) == 0
    assert _cabi.lib().s4g_close_region_f32(None, None, None, None, None, 1, 64, 2, 2 ** 31, 60, None, None, None, None,
                                            None, None, None, None, None, 0, None) == _cabi.S4G_EINVAL


def _regions_guarded_raw_resolution(dev, g2l, cloud, normals, R):
    """The C entry with a resolution the Python layer would refuse -> its return code; the outputs keep their sentinel."""
    from s4g_release_amd import _cabi
    from s4g_release_amd import functions as Fn
    B, F, N = g2l.shape[0], g2l.shape[1], cloud.shape[2]
    d_g, d_x, d_n = _t(g2l, dev), _t(cloud, dev), _t(normals, dev)
    params = (ctypes.c_float * 13)(-0.08, 0.09, 0.034, 0.012, *([1e-3] * 9))
    bufs = {k: _guarded(s, dev) for k, s in dict(count=(B, F), offset=(B, F + 1, 2), points=(B, 3, 64), normals=(B, 3, 64),
                                                 index=(B, 64), maps=(B, F, 12, 64, 64), flags=(B, F)).items()}
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    rc = _cabi.lib().s4g_close_region_f32(d_g.data_ptr(), d_x.data_ptr(), d_n.data_ptr(), None, None, B, N, F, 64, R,
                                          params, p["count"], p["offset"], p["points"], p["normals"], p["index"],
                                          p["maps"], p["flags"], ws.data_ptr(), ws.numel(), Fn._stream())
    torch.cuda.synchronize(dev)
    for k, (buf, _) in bufs.items():
        assert (buf == SENTINEL).all(), k
    return rc
