"""GPU tests of the fast baseline labels (`postprocess.grade_precomputed_baseline_frames`,
`label_precomputed_baseline_view`; the three-word sweep and `pvb_finish_kernel` of csrc/precomputed_view.hip) against
the fixture the reference's own `_find_match`, `finger_hand` and `close_region_projection` produced
(tests/golden/precomputed_baseline.npz), against the float64 yardstick (tests/precomputed_baseline_ref.py) and against
the shipped kernels: with all-zero scene labels
and the same mask, `grade_precomputed_frames` followed by `best_placement` must give the same bits.

The edge tests call the C ABI with every output and the workspace inside a poisoned buffer with guard bytes on both
sides, checked after the call.  Integers, booleans, the best index and the scores are compared exactly on the rows the
yardstick calls decided (every row of `lattice_scene`), the counts where no point lies within 4e-6 of a face;
`global_to_local` within 1e-5 (an fp32 product of a rotation and a roll, coordinates below 2: a few 2^-23), normals
within 1e-6, crop sets by `close_region_ref`'s rule (certain members in, ambiguous optional, nothing else), maps against
`projection64` of the call's own packed sets within `close_region_ref.map_bound`."""
import ctypes

import numpy as np
import pytest
import torch

from tests import close_region_ref as CRR
from tests import local_search_ref as LR
from tests import precomputed_baseline_ref as PB
from tests import precomputed_view_ref as PV

pytestmark = pytest.mark.gpu

GUARD = 256                # bytes on both sides of every output
POISON = 0xA5
COUNTS = ("back", "finger", "close")
GX, SLOTS = PB.slots_in_source()
P_ = GX * SLOTS            # frames of a scene per pass: the F ladder follows the source


def _t(a, dev):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cfg(**kw):
    from s4g_release_amd.postprocess import LocalSearchConfig, PrecomputedBaselineConfig
    base = {k: kw.pop(k) for k in list(kw) if k in ("antipodal_threshold", "sample_region")}
    return PrecomputedBaselineConfig(search=LocalSearchConfig(**kw), **base)


def _small_cfg():
    """2 depths x 3 rolls: the loop-edge shapes with hundreds of frames stay quick on the yardstick's side."""
    return _cfg(length_search=(-0.06, -0.02), theta_search_deg=(-30, 0, 30))


def _view_of(cfg):
    from s4g_release_amd.postprocess import PrecomputedViewConfig
    return PrecomputedViewConfig(search=cfg.search)


class _Guarded:
    def __init__(self, dev):
        self.dev, self.bufs = dev, {}

    def add(self, name, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.uint8, device=self.dev)
        self.bufs[name] = (buf, buf[GUARD:GUARD + n].view(dtype).view(shape), n)
        return self.bufs[name][1].data_ptr()

    def read(self, untouched=False):
        torch.cuda.synchronize(self.dev)
        out = {}
        for k, (buf, view, n) in self.bufs.items():
            assert (buf[:GUARD] == POISON).all() and (buf[GUARD + n:] == POISON).all(), "guard of %s" % k
            if untouched:
                assert (buf == POISON).all(), "%s was written" % k
            out[k] = view.cpu().numpy()
        return out


def _search_guarded(dev, points, frames, mask, pa, cloud, cfg, frame_count=None, expect=0, short=0):
    """s4g_precomputed_baseline_search_f32 through the C ABI, every output and the workspace guarded.  Batched numpy in
    -> dict of numpy arrays with the names of `precomputed_baseline_ref.grade64`.  short: bytes the workspace is
    declared too small by."""
    from s4g_release_amd import _cabi
    from s4g_release_amd import functions as Fn
    from s4g_release_amd.postprocess import _small_on_device
    s = cfg.search
    B, F = points.shape[:2]
    M = cloud.shape[2]
    L, T = s.shape
    ins = [_t(np.asarray(a, dt), dev) for a, dt in ((points, np.float32), (frames, np.float32), (mask, bool),
                                                    (pa, np.float32), (cloud, np.float32))]
    d_c = None if frame_count is None else _t(np.asarray(frame_count, np.int64), dev)
    tb = s.tables()
    tables = _small_on_device(torch.cat([tb["depth"], tb["lo"], tb["hi"], tb["cos"], tb["sin"]]), torch.float32, dev)
    params = (ctypes.c_float * 11)(s.finger_length, s.bottom_length, s.half_hand_thickness, s.half_bottom_width,
                                   s.half_bottom_space, s.back_collision_margin, s.back_collision_threshold,
                                   s.finger_collision_threshold, s.close_region_min_points,
                                   s.table_height + s.table_collision_offset, s.num_points_threshold)
    g = _Guarded(dev)
    p = {k: g.add(k, sh, dt) for k, sh, dt in (
        ("ints", (B, F, L, T, 4), torch.int32), ("scores", (B, F, L, T), torch.float32),
        ("slab_count", (B, F, L), torch.int32), ("index", (B, F), torch.int32), ("score", (B, F), torch.float32),
        ("g2l", (B, F, 4, 4), torch.float32), ("valid_index", (B, F), torch.int32), ("count", (B,), torch.int64))}
    nbytes = int(_cabi.lib().s4g_precomputed_baseline_search_workspace_bytes(B, M, F, L, T))
    ws = g.add("workspace", (max(nbytes, 1),), torch.uint8)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_precomputed_baseline_search_f32(
            *[a.data_ptr() for a in ins], B, M, F, L, T, params, tables.data_ptr(),
            None if d_c is None else d_c.data_ptr(), p["ints"], p["scores"], p["slab_count"], p["index"], p["score"],
            p["g2l"], p["valid_index"], p["count"], ws, nbytes - short, Fn._stream())
    assert rc == expect, rc
    out = g.read(untouched=expect != 0)
    for i, k in enumerate(("back", "finger", "close", "table_collision")):
        out[k] = out["ints"][..., i]
    return out


def _check_search(got, b, y, what, floor=1.0):
    """Scene b of a guarded result against `grade64`'s dict on the decided rows, at least `floor` of all."""
    keep = y["decided"]
    assert keep.mean() >= floor, (what, float(keep.mean()))
    r = np.nonzero(keep)[0]
    assert np.array_equal(got["table_collision"][b][r] != 0, y["table_collision"][r]), (what, "table")
    assert np.array_equal(got["scores"][b][r], y["scores"][r]), (what, "scores")
    clear = y["clear"][r]
    for k in COUNTS:
        assert np.array_equal(got[k][b][r][clear], y[k][r][clear].astype(np.int32)), (what, k)
    sure = y["amb_slab"][r] == 0
    assert np.array_equal(got["slab_count"][b][r][sure], y["slab_count"][r][sure].astype(np.int32)), (what, "slab")
    assert np.array_equal(got["index"][b][r], y["index"][r].astype(np.int32)), (what, "index")
    assert np.array_equal(got["score"][b][r], y["score"][r]), (what, "score")
    assert np.abs(got["g2l"][b][r] - y["g2l"][r]).max(initial=0.0) <= 1e-5, (what, "g2l")
    bad = got["index"][b] < 0
    assert not got["g2l"][b][bad].any() and not got["score"][b][bad].any(), (what, "invalid rows are zero")
    n = int(got["count"][b])
    assert np.array_equal(got["valid_index"][b][:n], np.nonzero(got["index"][b] >= 0)[0]), (what, "valid_index")
    assert (got["valid_index"][b][n:] == -1).all(), (what, "padding")
    if keep.all():
        assert n == y["count"] and np.array_equal(got["valid_index"][b], y["valid_index"].astype(np.int32)), what


def _lattice(rng, M, F, cfg, ties=True, **kw):
    """`precomputed_view_ref.lattice_scene` (decided under the view stage's gates, which include this class's) without
    the search scores; scores in eighths so that passing placements tie for the highest."""
    P, Fr, mask, _, pa, cloud, _ = PV.lattice_scene(rng, M, F, _view_of(cfg), **kw)
    if ties:
        pa = (np.ceil(pa * 8) / 8).astype(np.float32)
    return P, Fr, mask, pa, cloud


# ---- loop edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M,F", [(1, 3, 1), (1, 4, 2), (1, 1023, P_ - 1), (3, 1024, P_), (1, 1025, P_ + 1),
                                   (1, 63, 2 * P_ + 1), (1, 65535, 3), (3, 65536, 2), (1, 65537, 2)])
def test_search_edges(dev, B, M, F):
    """Chunk, sweep and pass boundaries; per-scene frame counts that differ and include 0; a NaN-padded scene tail."""
    cfg = _small_cfg() if F > 8 else _cfg()
    rng = np.random.default_rng(1000 * B + M + F)
    cases = [_lattice(rng, M, F, cfg, nan_from=M - M // 3 if b == 2 else None) for b in range(B)]
    counts = [F, 0, F // 2 + 1][:B] if B > 1 else [F]
    got = _search_guarded(dev, *[np.stack([c[i] for c in cases]) for i in range(5)], cfg,
                          frame_count=counts if B > 1 else None)
    for b, c in enumerate(cases):
        y = PB.grade64(*c, cfg, frame_count=counts[b])
        assert y["decided"].all()
        _check_search(got, b, y, (B, M, F, b))
        dead = np.arange(F) >= counts[b]
        assert (got["index"][b][dead] == -1).all() and not got["ints"][b][dead].any()
        assert not got["scores"][b][dead].any() and not got["slab_count"][b][dead].any()


def test_short_workspace(dev):
    cfg = _cfg()
    c = _lattice(np.random.default_rng(3), 200, 3, cfg)
    _search_guarded(dev, *[a[None] for a in c], cfg, expect=-2, short=1)      # S4G_EWORKSPACE, nothing written


def test_mask_and_frame_edges(dev):
    """(L, T) = (8, 16): an all-false row, single bits at placement 0, at L*T - 1 and on both sides of the 16-, 32- and
    64-placement boundaries, the zero frame in the middle of the list, a NaN scene point."""
    cfg = _cfg(length_search=tuple(-0.09 + 0.01 * i for i in range(8)), theta_search_deg=tuple(range(-88, 88, 11)))
    L, T = cfg.search.shape
    assert (L, T) == (8, 16)
    singles = [0, 15, 16, 31, 32, 63, 64, 127]
    F = len(singles) + 4
    rng = np.random.default_rng(5)
    mask = np.zeros((F, L, T), bool)
    for r, pl in enumerate(singles):
        mask[1 + r].reshape(-1)[pl] = True
    zero, full = len(singles) + 1, len(singles) + 2
    mask[zero] = mask[full] = mask[full + 1] = True
    P, Fr, mask, pa, cloud = _lattice(rng, 700, F, cfg, mask=mask, keep_rows=(zero,), nan_from=699)
    assert np.isnan(cloud[:, 699]).all()
    Fr[zero] = 0
    got = _search_guarded(dev, P[None], Fr[None], mask[None], pa[None], cloud[None], cfg)
    y = PB.grade64(P, Fr, mask, pa, cloud, cfg)
    assert y["decided"].all()
    _check_search(got, 0, y, "mask edges")
    for row in (0, zero):                                      # everything reads 0, the frame is invalid
        assert not got["ints"][0, row].any() and not got["scores"][0, row].any()
        assert not got["slab_count"][0, row].any() and got["index"][0, row] == -1
    for r, pl in enumerate(singles):                           # nothing outside the one open placement
        others = np.arange(L * T) != pl
        assert not got["ints"][0, 1 + r].reshape(L * T, 4)[others][:, :3].any(), pl
        assert got["index"][0, 1 + r] in (-1, pl)
    assert (got["index"][0, full:] >= 0).all()


def test_all_false_mask_reads_no_cloud(dev):
    """No mask bit in the whole call: no frame is scanned (the cloud may hold anything), every row reads zero."""
    cfg = _cfg()
    P, Fr, mask, pa, cloud = _lattice(np.random.default_rng(8), 300, 5, cfg)
    mask[:] = False
    cloud[:] = np.nan
    got = _search_guarded(dev, P[None], Fr[None], mask[None], pa[None], cloud[None], cfg)
    assert (got["index"] == -1).all() and int(got["count"][0]) == 0 and (got["valid_index"] == -1).all()
    assert not got["ints"][..., :3].any() and not got["scores"].any() and not got["slab_count"].any()
    assert not got["g2l"].any() and not got["score"].any()


def test_one_placement(dev):
    cfg = _cfg(length_search=(-0.04,), theta_search_deg=(0,))
    mask = np.ones((5, 1, 1), bool)
    mask[3] = False
    c = _lattice(np.random.default_rng(6), 300, 5, cfg, mask=mask)
    got = _search_guarded(dev, *[a[None] for a in c], cfg)
    y = PB.grade64(*c, cfg)
    assert y["valid"].sum() >= 2
    _check_search(got, 0, y, "(L, T) = (1, 1)")


def test_fold_takes_the_first_of_a_tie_and_skips_nan(dev):
    """Every placement open and passing on a blob scene; scores by hand: the maximum twice (the first wins), a NaN
    above a mask bit (never taken), a frame whose scores are all <= 0 (invalid)."""
    cfg = _cfg()
    L, T = cfg.search.shape
    rng = np.random.default_rng(9)
    P, Fr, mask, pa, cloud = _lattice(rng, 400, 6, cfg, mask=np.ones((6, L, T), bool))
    y0 = PB.grade64(P, Fr, mask, pa, cloud, cfg)
    passing = (y0["reason"] == 0).reshape(6, -1)
    assert (passing.sum(1) >= 3).all(), "the blob scene must leave three passing placements per frame"
    pa = np.full((6, L * T), 0.5, np.float32)
    want = []
    for f in range(6):
        a, b, c = np.nonzero(passing[f])[0][:3]
        if f < 3:                       # the maximum at the second and third passing placement: the second wins
            pa[f, [b, c]] = 0.875
            want.append(b)
        elif f == 3:                    # a NaN first: the next passing one is taken
            pa[f, a] = np.nan
            want.append(b)
        elif f == 4:                    # nothing positive
            pa[f] = -0.25
            want.append(-1)
        else:                           # a later, larger score replaces an earlier one
            pa[f, c] = 0.75
            want.append(c)
    pa = pa.reshape(6, L, T)
    got = _search_guarded(dev, P[None], Fr[None], mask[None], pa[None], cloud[None], cfg)
    assert got["index"][0].tolist() == want
    y = PB.grade64(P, Fr, mask, pa, cloud, cfg)
    assert y["index"].tolist() == want
    assert np.array_equal(got["g2l"][0][4], np.zeros((4, 4), np.float32))
    assert np.abs(got["g2l"][0] - y["g2l"]).max() <= 1e-5


# ---- against the shipped kernels ----------------------------------------------------------------------------------------
def _bits(s):
    b = s.best
    return [s.ints, s.scores, s.slab_count, b.index, b.score, b.global_to_local, b.valid_index, b.count]


@pytest.fixture(scope="module")
def box_case():
    cfg = _cfg()
    L, T = cfg.search.shape
    rng = np.random.default_rng(7)
    P, Fr, cloud, _, _ = LR.box_scene(rng, 6000, 96, cfg.search, n_boxes=4)
    F = len(P)
    mask = rng.random((F, L, T)) < 0.7
    mask[rng.random((F, L)) < 0.2] = False
    pa = (np.ceil(rng.uniform(0.3, 1, (F, L, T)) * 16) / 16).astype(np.float32)
    return cfg, P, Fr, mask, pa, cloud


def test_equals_the_composed_route(dev, box_case):
    """All-zero labels through `grade_precomputed_frames`, then `best_placement`: the parent's kernels on the same
    inputs.  back / finger / close / slab / scores and the whole best placement are bit-equal (the scores are above
    the mask's 0.3, so `best_placement`'s 1e-4 line, which this class does not have, rejects nothing)."""
    from s4g_release_amd import postprocess as PP
    cfg, P, Fr, mask, pa, cloud = box_case
    F, L, T = mask.shape
    d = [_t(a[None], dev) for a in (P, Fr, mask, pa, cloud)]
    new = PP.grade_precomputed_baseline_frames(*d, cfg)
    ps = torch.full((1, F, L, T), 100, dtype=torch.int32, device=dev)
    labels = torch.zeros((1, cloud.shape[1]), dtype=torch.int32, device=dev)
    old = PP.grade_precomputed_frames(d[0], d[1], d[2], ps, d[3], d[4], labels, _view_of(cfg))
    for k in ("back", "finger", "close", "table_collision"):
        assert torch.equal(getattr(new, k), getattr(old, k)), k
    assert torch.equal(new.slab_count, old.slab_count) and torch.equal(new.scores, old.scores)
    best = PP.best_placement(old._as_local())
    for k in ("index", "score", "global_to_local", "valid_index", "count"):
        assert torch.equal(getattr(new.best, k), getattr(best, k)), k
    n = int(new.best.count[0])
    assert 10 <= n < F, n
    idx = new.best.index[0].cpu().numpy()
    first = np.array([np.argmax(r) if r.any() else -1 for r in (new.scores[0].cpu().numpy().reshape(F, -1) > 0)])
    assert (idx[idx >= 0] != first[idx >= 0]).sum() >= 5, "the best placement is never a later one"


def test_properties(dev, box_case):
    """Two runs are bit-identical; a scene alone equals itself in a batch; one graph capture and replay equals the
    eager call; unbatched inputs get a leading 1."""
    from s4g_release_amd import postprocess as PP
    cfg, P, Fr, mask, pa, cloud = box_case
    d = [_t(a[None], dev) for a in (P, Fr, mask, pa, cloud)]
    one = PP.grade_precomputed_baseline_frames(*d, cfg)
    again = PP.grade_precomputed_baseline_frames(*d, cfg)
    assert all(torch.equal(a, b) for a, b in zip(_bits(one), _bits(again)))
    flat = PP.grade_precomputed_baseline_frames(*[a[0] for a in d], cfg)
    assert flat.unbatched and all(torch.equal(a, b) for a, b in zip(_bits(one), _bits(flat)))
    rng = np.random.default_rng(17)
    other = [rng.permutation(a, axis=0) if i < 4 else a[:, ::-1].copy() for i, a in enumerate((P, Fr, mask, pa, cloud))]
    three = [_t(np.stack([o, a, o]), dev) for a, o in zip((P, Fr, mask, pa, cloud), other)]
    cnt = _t(np.array([5, len(P), 0], np.int64), dev)
    batch = PP.grade_precomputed_baseline_frames(*three, cfg, frame_count=cnt)
    assert all(torch.equal(a[0], b[1]) for a, b in zip(_bits(one), _bits(batch)))
    assert int(batch.best.count[2]) == 0 and int((batch.best.index[0, 5:] >= 0).sum()) == 0
    run = lambda: PP.grade_precomputed_baseline_frames(*d, cfg)          # noqa: E731
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for t in _bits(out):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert all(torch.equal(a, b) for a, b in zip(_bits(one), _bits(out)))


# ---- the whole call -------------------------------------------------------------------------------------------------------
def _device_scene(sc, dev):
    from s4g_release_amd.postprocess import DarbouxScene
    return DarbouxScene(_t(sc["points"], dev), _t(sc["normals"], dev), _t(sc["labels"], dev), _t(sc["frames"], dev),
                        _t(sc["frames"], dev), _t(sc["search_score"], dev), _t(sc["inv_search_score"], dev),
                        _t(sc["antipodal_score"], dev), _t(sc["inv_antipodal_score"], dev))


def _view_case(seed, n_scene=3000, n_view=400):
    """`test_precomputed_view_gpu._view_case`'s recipe: a table-top scene with per-point frames [-n, -p, m] and
    synthetic scores, and a noisy view of it.  The search scores are all BELOW 50: the view-stage class would
    reject what this class, which does not read them, keeps."""
    cfg = _cfg()
    L, T = cfg.search.shape
    rng = np.random.default_rng(seed)
    _, _, cloud, nrm, lab = LR.box_scene(rng, n_scene, 1, cfg.search, n_boxes=3)
    M = cloud.shape[1]
    n = nrm.T.astype(np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    h = np.where(np.abs(n[:, 2:3]) < 0.9, [[0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0]])
    p = np.cross(n, h)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    frames = np.stack([-n, -p, np.cross(-n, -p)], 2).astype(np.float32)
    sc = {"points": cloud, "normals": nrm, "labels": lab, "frames": frames}
    for name in ("search_score", "inv_search_score"):
        sc[name] = rng.integers(0, 50, (M, L, T)).astype(np.int32)
    for name in ("antipodal_score", "inv_antipodal_score"):
        sc[name] = (np.ceil(rng.uniform(0, 1, (M, L, T)) * 16) / 16).astype(np.float32)
    pick = rng.choice(M, n_view)
    ref = cloud.T[pick].astype(np.float64) + rng.normal(0, 0.0008, (n_view, 3))
    ref[:12] += [0.0, 0.0, 0.5]                                          # strays: unmatched, but in the crop's cloud
    noisy = ref + rng.normal(0, 0.002, ref.shape)
    camera = np.array([0.5, -0.3, cfg.search.table_height + 0.8], np.float32)
    return cfg, sc, ref.T.astype(np.float32).copy(), noisy.T.astype(np.float32).copy(), camera


def test_whole_call_against_the_yardstick(dev):
    from s4g_release_amd import postprocess as PP
    cfg, sc, ref, noisy, camera = _view_case(11)
    m, g = PB.label64(ref, noisy, sc, camera, cfg, 0.01)
    v = PP.label_precomputed_baseline_view(_t(ref, dev), _t(noisy, dev), _device_scene(sc, dev), _t(camera, dev), cfg)
    assert isinstance(v, PP.PrecomputedBaselineLabels) and v.best is v.search.best
    kp, kf = PB.decided(m, g)
    assert kp.mean() > 0.97 and kf.mean() > 0.75, (float(kp.mean()), float(kf.mean()))
    assert m["flipped"].sum() > 50 and (m["nearest"] < 0).sum() >= 10 and g["count"] > 20
    mt = v.match
    assert np.array_equal(mt.nearest[0].cpu().numpy()[kp], m["nearest"][kp])
    assert np.abs(mt.normals[0].cpu().numpy().T - m["normals"])[kp].max() <= 1e-6
    assert np.array_equal(mt.flipped[0].cpu().numpy()[kp], m["flipped"][kp])
    assert np.array_equal(mt.pre_antipodal[0].cpu().numpy()[kp], m["pre_antipodal"][kp])
    assert np.array_equal(mt.mask[0].cpu().numpy()[kp], m["mask"][kp])
    assert np.array_equal(mt.candidate[0].cpu().numpy()[kp], m["candidate"][kp])
    # the mask is the antipodal threshold alone: the scene's search scores are all below 50
    assert (m["pre_search"] < 50).all() and m["mask"].any()
    fc = int(mt.frame_count[0])
    fi = mt.frame_index[0].cpu().numpy()
    row = {int(c): r for r, c in enumerate(fi[:fc])}
    yrows = np.array([r for r in np.nonzero(kf)[0] if int(m["frame_index"][r]) in row], int)
    assert len(yrows) == int(kf.sum())
    drows = np.array([row[int(m["frame_index"][r])] for r in yrows], int)
    s, best = v.search, v.best
    assert np.array_equal(s.scores[0].cpu().numpy()[drows], g["scores"][yrows])
    assert np.array_equal(s.table_collision[0].cpu().numpy()[drows] != 0, g["table_collision"][yrows])
    clear = g["clear"][yrows]
    for k in COUNTS:
        assert np.array_equal(getattr(s, k)[0].cpu().numpy()[drows][clear], g[k][yrows][clear].astype(np.int32)), k
    assert np.array_equal(best.index[0].cpu().numpy()[drows], g["index"][yrows].astype(np.int32))
    assert np.array_equal(best.score[0].cpu().numpy()[drows], g["score"][yrows])
    G = best.global_to_local[0].cpu().numpy()
    assert np.abs(G[drows] - g["g2l"][yrows]).max() <= 1e-5
    n = int(best.count[0])
    vi = best.valid_index[0].cpu().numpy()
    assert np.array_equal(vi[:n], np.nonzero(best.index[0].cpu().numpy() >= 0)[0]) and (vi[n:] == -1).all()
    ci = v.cloud_index[0].cpu().numpy()
    assert np.array_equal(ci[:n], fi[vi[:n]]) and (ci[n:] == -1).all()
    # the crop: the VIEW cloud with the matched, oriented normals in the best placement's frame, x in (0, finger_length)
    reg = CRR.regions64(G, noisy, cfg.search, (0.0, cfg.search.finger_length))
    cnt, off = v.regions.count[0].cpu().numpy(), v.regions.offset[0].cpu().numpy()
    assert not v.regions.flags[0].any()
    Pk, Nk, Ik = (t[0].cpu().numpy() for t in (v.regions.points, v.regions.normals, v.regions.index))
    maps = v.regions.maps[0].cpu().numpy()
    nrm32 = mt.normals[0].cpu().numpy()
    stray, empty = 0, 0
    for f in range(fc):
        r = reg[f]
        idx = Ik[off[f]:off[f + 1]]
        assert cnt[f] == len(idx) and (np.diff(idx) > 0).all()
        assert set(r["certain"]) <= set(idx) <= set(r["certain"]) | set(r["ambiguous"]), f
        if G[f].any() and len(idx) == 0:
            empty += 1                                                   # valid with an empty crop: kept, count 0
        if not len(idx):
            assert not maps[f].any()
            continue
        stray += int((m["nearest"][idx] < 0).sum())
        p32, n32 = Pk[:, off[f]:off[f + 1]], Nk[:, off[f]:off[f + 1]]
        assert np.abs(p32 - r["local"][:, idx]).max() < CRR.TOL
        want_n = G[f][:3, :3].astype(np.float64) @ nrm32[:, idx].astype(np.float64)
        assert np.abs(n32 - want_n).max() <= 1e-6
        own, _ = CRR.projection64(p32, n32, cfg.projection, cfg.search)
        assert (np.abs(maps[f] - own) <= CRR.map_bound(p32, n32, cfg.projection, cfg.search)).all(), f
    assert (cnt[fc:] == 0).all()
    d = v.dump(0, grasp_num=7)
    assert d["antipodal_score"].shape == (7,) and np.array_equal(d["valid_index"], ci[:7])
    assert np.array_equal(d["point_cloud"], noisy) and len(d["close_region_points_set"]) == 7
    assert np.abs(d["baseline_frame"] @ G[vi[:7]].astype(np.float64) - np.eye(4)).max() <= 1e-5
    full = v.dump(0)
    assert len(full["close_region_projection_map_set"]) == n and full["baseline_frame"].shape == (n, 4, 4)


def test_whole_call_is_repeatable_and_capturable(dev):
    """Two runs of the whole call are bit-identical, and one graph capture and replay equals the eager call."""
    from s4g_release_amd import postprocess as PP
    cfg, sc, ref, noisy, camera = _view_case(13, n_scene=1500, n_view=150)
    args = (_t(ref, dev), _t(noisy, dev), _device_scene(sc, dev), _t(camera, dev), cfg)
    bits = lambda v: _bits(v.search) + [v.match.mask, v.match.normals, v.match.frame_index, v.cloud_index,    # noqa: E731
                                        v.regions.count, v.regions.offset, v.regions.maps, v.regions.flags]
    one, again = PP.label_precomputed_baseline_view(*args), PP.label_precomputed_baseline_view(*args)
    assert int(one.best.count[0]) >= 5
    assert all(torch.equal(a, b) for a, b in zip(bits(one), bits(again)))
    n = int(one.regions.offset[0, -1])
    assert torch.equal(one.regions.points[..., :n], again.regions.points[..., :n])
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        PP.label_precomputed_baseline_view(*args)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = PP.label_precomputed_baseline_view(*args)
    for t in bits(out):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert all(torch.equal(a, b) for a, b in zip(bits(one), bits(out)))
    assert torch.equal(one.regions.points[..., :n], out.regions.points[..., :n])


def test_consumers_take_the_labels(dev):
    from s4g_release_amd import postprocess as PP
    cfg, sc, ref, noisy, camera = _view_case(12, n_scene=1500, n_view=120)
    v = PP.label_precomputed_baseline_view(_t(ref, dev), _t(noisy, dev), _device_scene(sc, dev), _t(camera, dev), cfg)
    seen = {}
    gpd = lambda maps, index=None: seen.update(maps=maps, index=index) or "gpd"             # noqa: E731
    pgpd = lambda pts, **kw: seen.update(points=pts, **kw) or "pointnetgpd"                 # noqa: E731
    assert PP.score_projections(v, gpd, grasp_num=5) == "gpd"
    assert seen["maps"] is v.regions.maps and torch.equal(seen["index"], v.best.valid_index[:, :5])
    assert PP.score_close_regions(v, pgpd, grasp_num=4) == "pointnetgpd"
    assert seen["points"] is v.regions.points and torch.equal(seen["index"], v.best.valid_index[:, :4])
    with pytest.raises(RuntimeError, match="PrecomputedBaselineLabels"):
        PP.score_projections(v.search, gpd)


def test_refusals(dev, box_case):
    from s4g_release_amd import _cabi
    from s4g_release_amd import postprocess as PP
    cfg, P, Fr, mask, pa, cloud = box_case
    d = [_t(a[None], dev) for a in (P, Fr, mask, pa, cloud)]
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        PP.grade_precomputed_baseline_frames(d[0].cpu(), *d[1:], cfg)
    with pytest.raises(RuntimeError, match="bool"):
        PP.grade_precomputed_baseline_frames(d[0], d[1], d[2].to(torch.uint8), d[3], d[4], cfg)
    with pytest.raises(RuntimeError, match="pre_antipodal"):
        PP.grade_precomputed_baseline_frames(d[0], d[1], d[2], d[3][:, :-1], d[4], cfg)
    with pytest.raises(ValueError):
        PP.grade_precomputed_baseline_frames(*d, _small_cfg())
    assert _cabi.lib().s4g_precomputed_baseline_search_workspace_bytes(1, 8, 1, 9, 4) == 0
    z = torch.zeros(64, device=dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_precomputed_baseline_search_f32(
            *[z.data_ptr()] * 5, 1, 8, 1, 9, 4, (ctypes.c_float * 11)(), z.data_ptr(), None, *[z.data_ptr()] * 8,
            z.data_ptr(), 0, None)
    assert rc == -1                                                      # S4G_EINVAL: L above the compiled maximum


# ---- the reference's own results ----------------------------------------------------------------------------------------
def test_fixture(dev):
    """tests/golden/precomputed_baseline.npz through the public call: every integer and boolean exact on the kept rows,
    `score` exact, `global_to_local` within 1e-5 of the reference's `valid_frame`, normals within 1e-6, crop sets by
    `close_region_ref`'s rule and equal to the reference's where no member is ambiguous, maps against the reference's
    outside `pixel_mask` within `map_bound` plus the fixture's margin."""
    from s4g_release_amd import postprocess as PP
    fx = PB.load_fixture()
    ref_cloud, cloud, sc, camera, cfg, radius = PB.case_of(fx)
    v = PP.label_precomputed_baseline_view(_t(ref_cloud, dev), _t(cloud, dev), _device_scene(sc, dev), _t(camera, dev),
                                           cfg, radius)
    kp, kf = fx["keep_points"].astype(bool), fx["keep_frames"].astype(bool)
    fi = fx["ref_frame_index"].astype(np.int64)
    mt, s, best = v.match, v.search, v.best
    assert np.abs(mt.normals[0].cpu().numpy().T - fx["ref_normals"])[kp].max() <= 1e-6
    cand = np.zeros(len(kp), bool)
    cand[fi] = True
    assert np.array_equal(mt.candidate[0].cpu().numpy()[kp], cand[kp])
    fc = int(mt.frame_count[0])
    dfi = mt.frame_index[0].cpu().numpy()
    row = {int(c): r for r, c in enumerate(dfi[:fc])}
    yrows = np.nonzero(kf)[0]
    assert all(int(fi[r]) in row for r in yrows)
    drows = np.array([row[int(fi[r])] for r in yrows], int)
    assert np.array_equal(mt.flipped[0].cpu().numpy()[fi[yrows]], fx["ref_flipped"][yrows])
    assert np.array_equal(mt.frames[0].cpu().numpy()[fi[yrows]], fx["ref_frames"][yrows])
    assert np.array_equal(mt.mask[0].cpu().numpy()[fi[yrows]], fx["ref_mask"][yrows])
    assert np.array_equal(mt.pre_antipodal[0].cpu().numpy()[fi[yrows]], fx["ref_pre_antipodal"][yrows])
    idx = best.index[0].cpu().numpy()
    assert np.array_equal(idx[drows] >= 0, fx["ref_valid"][yrows])
    assert np.array_equal(idx[drows], fx["ref_index"][yrows])
    assert np.array_equal(best.score[0].cpu().numpy()[drows], fx["ref_score"][yrows])
    G = best.global_to_local[0].cpu().numpy()
    assert np.abs(G[drows] - fx["ref_valid_frame"][yrows]).max() <= 1e-5
    n = int(best.count[0])
    vi = best.valid_index[0].cpu().numpy()
    ci = v.cloud_index[0].cpu().numpy()
    assert np.array_equal(vi[:n], np.nonzero(idx >= 0)[0]) and np.array_equal(ci[:n], dfi[vi[:n]])
    if kf.all() and kp.all():
        assert np.array_equal(ci[:n], fi[fx["ref_valid"]])                 # the reference's `valid_index` (:377)
    # the crop of the view
    off, cnt = v.regions.offset[0].cpu().numpy(), v.regions.count[0].cpu().numpy()
    Ik, Pk, Nk = (t[0].cpu().numpy() for t in (v.regions.index, v.regions.points, v.regions.normals))
    assert not v.regions.flags[0].any()
    reg = CRR.regions64(G, cloud, cfg.search, (0.0, cfg.search.finger_length))
    vrows = np.nonzero(fx["ref_valid"])[0]
    ro = fx["set_offset"]
    ref_set = {int(f): fx["set_index"][ro[k]:ro[k + 1]] for k, f in enumerate(vrows)}
    same = 0
    for r, d in zip(yrows, drows):
        got, want = Ik[off[d]:off[d + 1]], reg[d]
        assert cnt[d] == len(got)
        assert set(want["certain"]) <= set(got) <= set(want["certain"]) | set(want["ambiguous"]), r
        if fx["ref_valid"][r] and not fx["ref_ambiguous_crop"][r] and not len(want["ambiguous"]):
            assert np.array_equal(got, ref_set[int(r)]), r
            assert cnt[d] == fx["ref_set_size"][r]
            same += 1
    assert same >= 0.95 * fx["ref_valid"][yrows].sum()
    maps = v.regions.maps[0].cpu().numpy()
    so, compared = fx["stored_offset"], 0
    for k, r in enumerate(fx["stored_rows"]):
        d = row[int(fi[r])]
        got = Ik[off[d]:off[d + 1]]
        if not np.array_equal(got, ref_set[int(r)]):
            continue
        compared += 1
        p32, n32 = Pk[:, off[d]:off[d + 1]], Nk[:, off[d]:off[d + 1]]
        assert np.abs(p32 - fx["stored_points"][:, so[k]:so[k + 1]]).max(initial=0.0) < CRR.TOL
        assert np.abs(n32 - fx["stored_normals"][:, so[k]:so[k + 1]]).max(initial=0.0) <= 1e-5
        if not len(got):
            assert not maps[d].any() and not fx["maps"][k].any()
            continue
        bound = CRR.map_bound(p32, n32, cfg.projection, cfg.search)
        mask = CRR.pixel_mask(reg[d]["local"][:, got], cfg.projection, cfg.search)
        dist = np.abs(maps[d].astype(np.float64) - fx["maps"][k])
        assert (dist <= bound + float(fx["margin"][0]))[~mask].all(), (r, float((dist * ~mask).max()))
    assert compared >= 20
