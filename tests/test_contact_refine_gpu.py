"""The refine and reduce stages of the contact-object pipeline on the device (`contact_object.refine_contact_frames`,
`reduce_contact_frames`, `refine_contact_object`, `reduce_contact_object`; csrc/contact_refine.hip and
s4g_match_knn_f32) against what the reference's own scripts wrote (tests/golden/contact_refine.npz) and the float64
yardstick of tests/contact_refine_ref.py (checked on the CPU by tests/test_contact_refine_ref.py).

Tolerances: none.  Every compared value is an integer.  On the fixture the refine stage is compared on the rows the
yardstick calls decided at the fixture's own eps (kept, score, failure bits) and exact (every count word); the reduce
stage holds integers and one neighbour search whose fp32 order equals the float64 order on every querying point of
the fixture (asserted on the CPU), so it is compared whole.

The refine edge scenes sit on a 1 / 2048 m lattice with axis-aligned frames and lattice translations: every local
coordinate is exact in fp32 and none is 0 (odd point values, even translations), and no bound of any placement used
is within 1e-5 m of a lattice value, so EVERY row is exact there (asserted per scene with eps 2e-6).  The reduce edge clouds are points on a line 1 / 256 m apart (4 / 1024):
squared distances are exact in fp32, ties are exact ties, and the neighbour lists are known by construction."""
import ctypes

import numpy as np
import pytest
import torch

from tests import contact_refine_ref as CR
from tests import golden_util as GU

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -559038737
STEP = 1.0 / 2048
LANE_BLOCK = 1024                          # csrc/contact_refine.hip: 256 lanes x CR_U
FULL_PASS = 64 * 13                        # CR_GX x CR_SLOTS
CHUNK_POINTS, MIN_CHUNKS = 16384, 4
LIST4 = (-0.01, 0.01, 0, 0.005)
WIDTH4 = (-0.002, 0.002, 0, 0.001)        # (a width shift of 0.01 would put the whole strip into a finger)
EDGE_EPS = 2e-6
LINE = 4.0 / 1024


def _t(a, dev):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _guarded(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _read(bufs, floats=(), longs=()):
    out = {}
    for k, (buf, view) in bufs.items():
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "guard of %s" % k
        a = view.cpu().numpy()
        if k in floats:
            a = a.view(np.float32)
        if k in longs:
            a = a.view(np.int64)[..., 0]
        out[k] = a
    return out


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _refine_guarded(dev, xyz, g2l, search, cfg=None, count=None, frame_count=None, expect_rc=0):
    """s4g_contact_refine_f32 through the C ABI with every output and the workspace inside guarded buffers."""
    from s4g_release_amd import _cabi, contact_object as CO, postprocess as PP
    from s4g_release_amd import functions as Fn
    cfg = cfg or CO.ContactRefineConfig()
    B, _, M = xyz.shape
    F = g2l.shape[1]
    nz, ny, nx = cfg.shape
    P = cfg.placements
    d = [_t(np.asarray(a, np.float32), dev) for a in (xyz, g2l, search)]
    d_c = None if count is None else _t(np.asarray(count, np.int64), dev)
    d_f = None if frame_count is None else _t(np.asarray(frame_count, np.int64), dev)
    tb = cfg.tables()
    tables = PP._small_on_device(torch.cat([tb[k] for k in ("zlo", "zhi", "ylo", "yhi", "dy", "xlo", "xhi")]),
                                 torch.float32, dev)
    bufs = {k: _guarded(s, dev) for k, s in (("counts", (B, F, P, 3)), ("kept", (B, F)), ("score", (B, F)),
                                             ("fail", (B, F)), ("kept_index", (B, F)), ("kept_count", (B, 2)))}
    params = (ctypes.c_float * 8)(cfg.finger_length, cfg.bottom_length, cfg.half_hand_thickness, cfg.half_bottom_width,
                                  cfg.half_bottom_space, max(abs(float(v)) for v in cfg.length_search),
                                  max(abs(float(v)) for v in cfg.width_search),
                                  max(abs(float(v)) for v in cfg.height_search))
    nbytes = int(_cabi.lib().s4g_contact_refine_workspace_bytes(B, M, F, P))
    ws = torch.full((nbytes + 2 * GUARD * 4,), 0x5A, dtype=torch.uint8, device=dev)
    rc = _cabi.lib().s4g_contact_refine_f32(
        _ptr(d[1]), d[0].data_ptr(), _ptr(d[2]), B, M, F, nz, ny, nx, params, int(cfg.min_search_score),
        int(cfg.collision_threshold), tables.data_ptr(), _ptr(d_c), _ptr(d_f),
        *[_ptr(bufs[k][1]) for k in ("counts", "kept", "score", "fail", "kept_index")], bufs["kept_count"][1].data_ptr(),
        ws[GUARD * 4:].data_ptr(), nbytes, Fn._stream())
    assert rc == expect_rc, rc
    torch.cuda.synchronize(dev)
    assert (ws[:GUARD * 4] == 0x5A).all() and (ws[GUARD * 4 + nbytes:] == 0x5A).all(), "guard of the workspace"
    if expect_rc != 0:
        for k, (buf, _) in bufs.items():
            assert (buf == SENTINEL).all(), "a refused call wrote %s" % k
        return None
    return _read(bufs, floats=("score",), longs=("kept_count",))


def _reduce_guarded(dev, xyz, fpi, search, cfg=None, count=None, frame_count=None, cap=None, expect_rc=0):
    """s4g_match_knn_f32 and s4g_contact_reduce_i32 through the C ABI on guarded buffers, the CSR formed as
    `reduce_contact_frames` forms it."""
    from s4g_release_amd import _cabi, contact_object as CO, postprocess as PP
    from s4g_release_amd import functions as Fn
    cfg = cfg or CO.ContactReduceConfig()
    B, _, N = xyz.shape
    F = fpi.shape[1]
    if cap is None:
        cap = min(F, N * cfg.frame_per_point)
    d_x, d_s = _t(np.asarray(xyz, np.float32), dev), _t(np.asarray(search, np.float32), dev)
    d_i = _t(np.asarray(fpi, np.int32), dev)
    d_c = None if count is None else _t(np.asarray(count, np.int64), dev)
    d_f = None if frame_count is None else _t(np.asarray(frame_count, np.int64), dev)
    lim = N if d_c is None else d_c.view(B, 1)
    dead = ~(d_s > float(cfg.min_search_score)) | (d_i < 0) | (d_i >= lim)
    fpi32 = torch.where(dead, d_i.new_full((), -1), d_i).contiguous()
    offsets, order = PP.frames_by_point(fpi32, N, d_f)
    live = None if d_c is None else d_c.clamp(0, N).to(torch.int32)
    bufs = {k: _guarded(s, dev) for k, s in (("knn", (B, N, cfg.max_nn)), ("source", (B, cap)), ("point", (B, cap)),
                                             ("count", (B, 2)), ("flags", (B,)))}
    nbytes = int(_cabi.lib().s4g_estimate_normals_workspace_bytes(B, N))
    ws = torch.full((nbytes + 2 * GUARD * 4,), 0x5A, dtype=torch.uint8, device=dev)
    rc = _cabi.lib().s4g_match_knn_f32(d_x.data_ptr(), _ptr(live), B, N, float(cfg.radius), int(cfg.max_nn),
                                       bufs["knn"][1].data_ptr(), ws[GUARD * 4:].data_ptr(), nbytes, Fn._stream())
    assert rc == 0, rc
    rc = _cabi.lib().s4g_contact_reduce_i32(
        _ptr(fpi32), offsets.data_ptr(), _ptr(order), bufs["knn"][1].data_ptr(), _ptr(d_c), B, N, F,
        int(cfg.frame_per_point), int(cfg.max_neighbor_frame), int(cfg.min_rest), int(cfg.max_nn), cap,
        _ptr(bufs["source"][1]), _ptr(bufs["point"][1]), bufs["count"][1].data_ptr(), bufs["flags"][1].data_ptr(),
        Fn._stream())
    assert rc == expect_rc, rc
    torch.cuda.synchronize(dev)
    assert (ws[:GUARD * 4] == 0x5A).all() and (ws[GUARD * 4 + nbytes:] == 0x5A).all(), "guard of the workspace"
    if expect_rc != 0:
        for k in ("source", "point", "count", "flags"):
            assert (bufs[k][0] == SENTINEL).all(), "a refused call wrote %s" % k
        return None
    return _read(bufs, longs=("count",))


def _cf(a):
    """(N, 3) -> (1, 3, N) contiguous"""
    return np.ascontiguousarray(np.asarray(a, np.float32).T[None])


# ---- fixtures ----

@pytest.fixture(scope="module")
def fx():
    g, r = GU.load("contact_pairs.npz"), GU.load("contact_refine.npz")
    out = {k: g[k] for k in g.files}
    out.update({"r_" + k: r[k] for k in r.files})
    return out


@pytest.fixture(scope="module")
def yard(fx):
    return CR.refine(fx["points"], fx["global_to_local"], fx["search_score"], eps=float(fx["r_eps"][0]))


@pytest.fixture(scope="module")
def stage1(dev, fx):
    """The reference's stage-1 output as an object with `ObjectContactFrames`' attributes."""
    from types import SimpleNamespace
    F = len(fx["search_score"])
    return SimpleNamespace(
        points=_t(_cf(fx["points"]), dev), normals=_t(_cf(fx["normals"]), dev), count=None,
        global_to_local=_t(fx["global_to_local"][None], dev), search_score=_t(fx["search_score"][None], dev),
        antipodal_score=_t(fx["antipodal_score"].astype(np.float32)[None], dev),
        frame_point_index=_t(fx["frame_point_index"][None], dev),
        frame_count=torch.tensor([F], dtype=torch.int64, device=dev),
        flags=torch.zeros(1, dtype=torch.int32, device=dev), unbatched=True)


def _check_refine(got, b, y, F=None, what=""):
    """Object b of a guarded refine result against the yardstick: decided rows for the verdict, exact rows for the
    counts, the compaction against the device's own kept flags."""
    F = len(y["kept"]) if F is None else F
    d, e = y["decided"][:F], y["exact"][:F]
    assert np.array_equal(got["kept"][b, :F][d] != 0, y["kept"][:F][d]), what
    assert np.array_equal(got["score"][b, :F][d], y["score"][:F][d].astype(np.float32)), what
    assert np.array_equal(got["fail"][b, :F][d], y["fail"][:F][d]), what
    assert np.array_equal(got["counts"][b, :F][e], y["counts"][:F][e]), what
    rows = np.nonzero(got["kept"][b])[0]
    assert got["kept_count"][b] == len(rows), what
    assert np.array_equal(got["kept_index"][b, :len(rows)], rows) and (got["kept_index"][b, len(rows):] == -1).all(), what
    assert np.array_equal(got["kept"][b] != 0, got["fail"][b] == 0), what


# ---- the fixture ----

def test_fixture_refine(dev, fx, yard):
    got = _refine_guarded(dev, _cf(fx["points"]), fx["global_to_local"][None], fx["search_score"][None])
    _check_refine(got, 0, yard, what="fixture")
    ref = np.zeros(len(yard["kept"]), bool)
    ref[fx["r_kept_index"]] = True
    d = yard["decided"]
    assert np.array_equal(got["kept"][0][d] != 0, ref[d])                 # the reference's own kept set
    both = d & ref
    score = np.zeros(len(ref))
    score[fx["r_kept_index"]] = fx["r_search_score"]
    assert np.array_equal(got["score"][0][both], score[both].astype(np.float32))
    assert both.sum() >= 2000 and yard["exact"].mean() > 0.8


@pytest.mark.parametrize("k", [0, 1])
def test_fixture_reduce_from_the_reference_refine_output(dev, fx, k):
    from s4g_release_amd import contact_object as CO
    fpp, mnf = (int(v) for v in fx["r_settings"][k])
    cfg = CO.ContactReduceConfig(frame_per_point=fpp, max_neighbor_frame=mnf)
    got = _reduce_guarded(dev, _cf(fx["points"]), fx["r_frame_point_index"][None],
                          fx["r_search_score"].astype(np.float32)[None], cfg)
    src, pts = fx["r_reduce_%d_%d_source" % (fpp, mnf)], fx["r_reduce_%d_%d_point" % (fpp, mnf)]
    n = len(src)
    assert got["count"][0] == n and got["flags"][0] == 0
    assert np.array_equal(got["source"][0, :n], src) and np.array_equal(got["point"][0, :n], pts)
    assert (got["source"][0, n:] == -1).all() and (got["point"][0, n:] == -1).all()


def test_fixture_objects_and_chain(dev, fx, yard, stage1):
    """`refine_contact_object` / `reduce_contact_object`: the dump against the reference's dictionary on the decided
    rows, and refine -> reduce against the yardstick's reduce of the library's own refine output."""
    from s4g_release_amd import contact_object as CO
    from s4g_release_amd import postprocess as PP
    ref = CO.refine_contact_object(stage1)
    dump = ref.dump(0)
    kept = ref.stage.kept_index[0, :int(ref.frame_count[0])].cpu().numpy()
    assert dump["search_score"].dtype == np.int64 and dump["frame_point_index"].dtype == np.int64
    assert dump["global_to_local"].dtype == np.float32 and dump["cloud"].shape == fx["points"].shape
    assert np.array_equal(dump["global_to_local"], fx["global_to_local"][kept])
    assert np.array_equal(dump["frame_point_index"], fx["frame_point_index"][kept])
    assert np.array_equal(dump["antipodal_score"], fx["antipodal_score"].astype(np.float32)[kept])
    d = yard["decided"]
    assert np.array_equal(kept[d[kept]], fx["r_kept_index"][d[fx["r_kept_index"]]])
    pos = {f: i for i, f in enumerate(fx["r_kept_index"])}
    rows = [i for i, f in enumerate(kept) if d[f] and f in pos]
    assert np.array_equal(dump["search_score"][rows], fx["r_search_score"][[pos[kept[i]] for i in rows]])
    assert (ref.frame_point_index[0, len(kept):] == -1).all() and (ref.search_score[0, len(kept):] == 0).all()
    for fpp, mnf in ((5, 4), (2, 1)):
        red = CO.reduce_contact_object(ref, CO.ContactReduceConfig(frame_per_point=fpp, max_neighbor_frame=mnf))
        y = CR.reduce(fx["points"], dump["frame_point_index"], dump["search_score"], frame_per_point=fpp,
                      max_neighbor_frame=mnf)
        n = int(red.frame_count[0])
        assert n == len(y["source_frame"]) and int(red.flags[0]) == 0
        assert np.array_equal(red.stage.source_frame[0, :n].cpu().numpy(), y["source_frame"])
        assert np.array_equal(red.frame_point_index[0, :n].cpu().numpy(), y["point_index"])
        out = red.dump(0)
        assert np.array_equal(out["global_to_local"], dump["global_to_local"][y["source_frame"]])
        assert np.array_equal(out["search_score"], dump["search_score"][y["source_frame"]])
        assert np.array_equal(out["antipodal_score"], dump["antipodal_score"][y["source_frame"]])
    scene = PP.compose_contact_scene([red], [(0.0, 0.0, 0.8, 1.0, 0.0, 0.0, 0.0)])
    assert scene.global_to_local.shape[0] == n and int(scene.frame_point_index.max()) < fx["points"].shape[0]


def test_counts_equal_grade_contact_frames(dev, fx):
    """The three count words are grade_contact_frames' finger / close / behind integers on the same lists."""
    from s4g_release_amd import contact_object as CO
    from s4g_release_amd import postprocess as PP
    cfg = CO.ContactRefineConfig()
    xyz, g2l = _t(_cf(fx["points"]), dev), _t(fx["global_to_local"][None], dev)
    r = CO.refine_contact_frames(xyz, g2l, _t(fx["search_score"][None], dev), cfg)
    s = PP.grade_contact_frames(g2l, xyz, torch.zeros((1, xyz.shape[2]), dtype=torch.int32, device=dev),
                                PP.ContactSearchConfig(width_search=cfg.width_search, height_search=cfg.height_search,
                                                       length_search=cfg.length_search, back_collision_margin=0.0))
    live = (r.fail[0] & CO.REFINE_FAIL_FILTERED) == 0
    assert int(live.sum()) == (fx["search_score"] > 100).sum()
    assert torch.equal(r.counts[0][live], s.ints[0][live][..., :3])
    assert (r.counts[0][~live] == 0).all()


# ---- refine edges: lattice scenes ----

def lattice_scene(seed, M, F, nan_points=0, min_score=3):
    """M lattice points -- a strip between the fingers in front of the palm and up to 6 strays beside the fingers -- and
    F axis-aligned frames with lattice translations: small ones, which keep the frame, and per eight frames one that
    moves the strip into a finger, one behind the palm, one out of the hand's thickness and one with permuted axes.
    Scores around min_score."""
    rng = np.random.default_rng(seed)
    P = np.stack([rng.integers(10, 75, M), rng.integers(-30, 30, M), rng.integers(-40, 41, M)], 1) * 2 + 1
    k = min(M // 3, 6)
    P[:k] = np.stack([rng.integers(-40, 90, k) * 2 + 1, rng.choice([-1, 1], k) * (rng.integers(63, 69, k) * 2 + 1),
                      rng.integers(-3, 3, k) * 2 + 1], 1)
    P = (P[rng.permutation(M)] * STEP).astype(np.float32)   # odd lattice values, even translations: no coordinate is 0
    if nan_points:
        P[rng.choice(M, nan_points, replace=False), rng.integers(0, 3, nan_points)] = \
            np.where(np.arange(nan_points) % 3 == 0, np.nan, np.where(np.arange(nan_points) % 3 == 1, np.inf, -np.inf))
    G = np.zeros((F, 4, 4), np.float32)
    for f in range(F):
        kind = f % 8
        perm = rng.permutation(3) if kind == 7 else np.arange(3)
        G[f, np.arange(3), perm] = rng.choice([-1.0, 1.0], 3) if kind == 7 else 1.0
        t = rng.integers(-3, 6, 3) * 2 * (kind != 0)
        if kind == 4:
            t[1] = rng.choice([-1, 1]) * 2 * rng.integers(20, 40)
        if kind == 5:
            t[0] = -2 * rng.integers(8, 30)
        if kind == 6:
            t[2] = rng.choice([-1, 1]) * 2 * rng.integers(5, 40)
        G[f, :3, 3] = t * STEP
        G[f, 3, 3] = 1.0
    m = float(min_score)
    search = rng.choice([m - 1, m, m + 0.5, m + 1, 250.0, 250.0, 250.0, 250.0], F).astype(np.float32)
    return P, G, search


def _edge_cfg(lists=None, **kw):
    from s4g_release_amd import contact_object as CO
    if lists is not None:
        kw.update(height_search=lists[0], width_search=lists[1], length_search=lists[2])
    kw.setdefault("min_search_score", 3)
    return CO.ContactRefineConfig(**kw)


def _edge_yard(P, G, search, cfg, points=None, frames=None, eps=EDGE_EPS):
    """The yardstick on the points / rows that count, every row exact; rows past `frames` read filtered."""
    n = len(P) if points is None else points
    F = len(G) if frames is None else frames
    with np.errstate(invalid="ignore", over="ignore"):
        y = CR.refine(P[:n].astype(np.float64), G[:F], search[:F], min_search_score=cfg.min_search_score,
                      collision_threshold=cfg.collision_threshold, heights=cfg.height_search, widths=cfg.width_search,
                      lengths=cfg.length_search, eps=eps)
    assert y["decided"].all() and y["exact"].all()
    pad = len(G) - F
    if pad:
        y = {"kept": np.r_[y["kept"], np.zeros(pad, bool)], "score": np.r_[y["score"], np.zeros(pad, np.int64)],
             "fail": np.r_[y["fail"], np.full(pad, CR.FAIL_FILTERED)], "decided": np.ones(len(G), bool),
             "exact": np.ones(len(G), bool),
             "counts": np.concatenate([y["counts"], np.zeros((pad,) + y["counts"].shape[1:], np.int64)])}
    return y


POINT_EDGES = [1, 255, 256, 257, LANE_BLOCK - 1, LANE_BLOCK, LANE_BLOCK + 1, 4 * LANE_BLOCK - 1, 4 * LANE_BLOCK,
               4 * LANE_BLOCK + 1, MIN_CHUNKS * CHUNK_POINTS, MIN_CHUNKS * CHUNK_POINTS + 1]


@pytest.mark.parametrize("M", POINT_EDGES)
def test_refine_point_edges(dev, M):
    """M = 1, either side of a wave block, of a lane block (256 x 4 points), of a chunk that ends on one, and of the
    point count at which a fifth chunk appears."""
    P, G, search = lattice_scene(M, M, 24)
    cfg = _edge_cfg()
    y = _edge_yard(P, G, search, cfg)
    assert M == 1 or 0 < y["kept"].sum() < len(G)
    _check_refine(_refine_guarded(dev, _cf(P), G[None], search[None], cfg), 0, y, what=M)


@pytest.mark.parametrize("F", [0, 1, FULL_PASS - 1, FULL_PASS, FULL_PASS + 1])
def test_refine_frame_edges(dev, F):
    P, G, search = lattice_scene(F + 7, 300, F)
    cfg = _edge_cfg()
    got = _refine_guarded(dev, _cf(P), G[None], search[None], cfg)
    if F == 0:
        assert got["kept_count"][0] == 0
        return
    y = _edge_yard(P, G, search, cfg)
    assert F == 1 or 0 < y["kept"].sum() < F
    _check_refine(got, 0, y, what=F)


@pytest.mark.parametrize("lists", [((0,), (0,), (0,)), (LIST4, WIDTH4, LIST4), ((0,), (0.005, 0), (0,))])
def test_refine_shift_lists(dev, lists):
    """1 x 1 x 1, 4 x 4 x 4, and a one-sided width list, where the sign of dy shows."""
    P, G, search = lattice_scene(11, 700, 40)
    cfg = _edge_cfg(lists)
    y = _edge_yard(P, G, search, cfg)
    assert 0 < y["kept"].sum() < len(G) and y["counts"].shape[1] == cfg.placements
    _check_refine(_refine_guarded(dev, _cf(P), G[None], search[None], cfg), 0, y, what=lists)
    if len(lists[1]) == 2:
        with np.errstate(invalid="ignore"):
            bad = CR.refine(P.astype(np.float64), G, search, min_search_score=3, heights=lists[0], widths=lists[1],
                            lengths=lists[2], sabotage="dy_sign")
        assert (bad["counts"] != y["counts"]).any()


def test_refine_filtered_rows_frame_count_and_nonfinite(dev):
    """All rows filtered; frame_count 0 and partial; a NaN frame between live ones; NaN / inf points; a point count."""
    from s4g_release_amd import contact_object as CO
    P, G, search = lattice_scene(5, 600, 50, nan_points=9)
    cfg = _edge_cfg()
    got = _refine_guarded(dev, _cf(P), G[None], np.full((1, 50), float(cfg.min_search_score), np.float32), cfg)
    assert (got["fail"] == CO.REFINE_FAIL_FILTERED).all() and got["kept_count"][0] == 0 and (got["counts"] == 0).all()
    assert (got["kept_index"] == -1).all() and (got["score"] == 0).all()
    got = _refine_guarded(dev, _cf(P), G[None], search[None], cfg, frame_count=[0])
    assert (got["fail"] == CO.REFINE_FAIL_FILTERED).all() and got["kept_count"][0] == 0
    search[:] = 250.0
    search[7] = np.nan
    G[20, 1, 3] = np.nan
    G[21, 3, 0] = np.inf
    y = _edge_yard(P, G, search, cfg, frames=33)
    assert y["fail"][7] == CR.FAIL_FILTERED and y["fail"][20] == y["fail"][21] == CR.FAIL_NONFINITE
    assert y["kept"][19] or y["kept"][22] or y["kept"].sum() > 3
    _check_refine(_refine_guarded(dev, _cf(P), G[None], search[None], cfg, frame_count=[33]), 0, y, what="partial")
    y = _edge_yard(P, G, search, cfg, points=401)
    _check_refine(_refine_guarded(dev, _cf(P), G[None], search[None], cfg, count=[401]), 0, y, what="count")


def test_refine_threshold_count_gate_and_x_zero(dev):
    """collision_threshold 3 (post_process_single_grasp.py's constants: one placement); a close region of exactly
    min_search_score points against one fewer; a close point at exactly x = 0 is not behind, one lattice step behind
    it is.  (Identity frames: the coordinates are the lattice values themselves, and the yardstick runs without eps,
    which would call x = 0 undecided.)"""
    G = np.eye(4, dtype=np.float32)[None].repeat(2, 0)
    close = np.stack([np.arange(6) * 4 * STEP, np.zeros(6), np.zeros(6)], 1)          # x = 0 is among them
    finger = np.stack([np.full(4, 20 * STEP), np.full(4, 90 * STEP), np.arange(4) * STEP], 1)
    search = np.full(2, 250.0, np.float32)
    for nf, thr, nclose, shift, fail in ((3, 3, 6, 0, 0), (4, 3, 6, 0, CR.FAIL_FINGER), (0, 0, 5, 0, CR.FAIL_FEW),
                                         (0, 0, 6, -1, CR.FAIL_BEHIND), (1, 0, 6, 0, CR.FAIL_FINGER)):
        P = np.concatenate([close[:nclose] + [shift * STEP, 0, 0], finger[:nf]]).astype(np.float32)
        cfg = _edge_cfg(((0,), (0,), (0,)), min_search_score=6, collision_threshold=thr)
        y = _edge_yard(P, G, search, cfg, eps=0.0)
        assert (y["fail"] == fail).all(), (nf, thr, nclose, shift)
        _check_refine(_refine_guarded(dev, _cf(P), G[None], search[None], cfg), 0, y, what=(nf, thr, nclose, shift))


# ---- reduce edges: points on a line ----

def line_case(seed, N, counts=None, duplicates=(), low_share=0.2):
    """N points on a line LINE apart (duplicates: (j, i) makes point j a copy of point i), frames per point from
    `counts` (cycled), a share of them at or below the filter, given in shuffled order."""
    rng = np.random.default_rng(seed)
    P = np.zeros((N, 3), np.float32)
    P[:, 0] = np.arange(N) * LINE
    for j, i in duplicates:
        P[j] = P[i]
    counts = [0, 1, 5, 6, 10, 11, 3, 12, 0, 7, 11, 2, 14, 5, 11, 11] if counts is None else counts
    fpi = np.concatenate([np.full(counts[i % len(counts)], i) for i in range(N)] + [np.zeros(0, int)]).astype(np.int32)
    fpi = fpi[rng.permutation(len(fpi))]
    search = np.where(rng.random(len(fpi)) < low_share, rng.choice([50.0, 49.0, 3.0], len(fpi)),
                      rng.integers(51, 400, len(fpi))).astype(np.float32)
    return P, fpi, search


def _check_reduce(got, b, P, fpi, search, cfg, cap=None, what=""):
    y = CR.reduce(P.astype(np.float64), fpi, search, cfg.min_search_score, cfg.frame_per_point, cfg.max_neighbor_frame,
                  cfg.min_rest, cfg.radius, cfg.max_nn)
    K = len(y["source_frame"])
    cap = got["source"].shape[1] if cap is None else cap
    n = min(K, cap)
    assert got["count"][b] == K, (what, got["count"][b], K)              # exact, also when the list does not fit
    assert got["flags"][b] == (1 if K > cap else 0), what
    assert np.array_equal(got["source"][b, :n], y["source_frame"][:n]), what
    assert np.array_equal(got["point"][b, :n], y["point_index"][:n]), what
    assert (got["source"][b, n:] == -1).all() and (got["point"][b, n:] == -1).all(), what
    for i in range(len(P)):                                               # every neighbour list, known by construction
        want = CR.knn(P.astype(np.float64), i, cfg.radius, cfg.max_nn)
        assert np.array_equal(got["knn"][b, i, :len(want)], want) and (got["knn"][b, i, len(want):] == -1).all(), (what, i)
    return y


def test_reduce_line_covers_every_branch(dev):
    """Fewer than max_nn neighbours (the line's ends), exactly frame_per_point frames and one more, a rest of exactly
    min_rest and one more, a full lower neighbour, a higher neighbour at its cap, points already holding frames,
    frames in arbitrary point order and below the filter."""
    from s4g_release_amd import contact_object as CO
    total = {}
    for seed, (fpp, mnf) in ((1, (5, 4)), (2, (2, 1))):     # (a higher neighbour reaches a cap of 4 only among duplicates)
        cfg = CO.ContactReduceConfig(frame_per_point=fpp, max_neighbor_frame=mnf)
        P, fpi, search = line_case(seed, 48, low_share=0.1 * seed)
        y = _check_reduce(_reduce_guarded(dev, _cf(P), fpi[None], search[None], cfg), 0, P, fpi, search, cfg, what=seed)
        for k, v in y["stats"].items():
            total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total
    cfg = CO.ContactReduceConfig()
    assert len(CR.knn(P.astype(np.float64), 0)) == 3 and len(CR.knn(P.astype(np.float64), 1)) == 4
    # exact boundaries on unfiltered frames: 5 | 6 frames, rests of 5 | 6
    for counts, spread in (([5] * 8, 0), ([6] * 8, 0), ([0, 0, 0, 10, 0, 0, 0, 0], 0), ([0, 0, 0, 11, 0, 0, 0, 0], 4)):
        P, fpi, search = line_case(3, 8, counts, low_share=0.0)
        y = _check_reduce(_reduce_guarded(dev, _cf(P), fpi[None], search[None], cfg), 0, P, fpi, search, cfg, what=counts)
        assert y["stats"]["spread"] == spread, counts


def test_reduce_duplicates_small_shapes_and_caps(dev):
    """Duplicate points, including a lower-index copy of the querying point (which ranks before it and takes rest[0]);
    N = 1; F = 0; every frame on one point; a capacity overflow; frame_per_point 1 and 255; indices out of range."""
    from s4g_release_amd import contact_object as CO
    cfg = CO.ContactReduceConfig()
    P, fpi, search = line_case(4, 12, [0, 0, 2, 0, 0, 14, 0, 0, 0, 12, 0, 0], duplicates=((4, 5), (10, 9)), low_share=0.0)
    y = _check_reduce(_reduce_guarded(dev, _cf(P), fpi[None], search[None], cfg), 0, P, fpi, search, cfg, what="dup")
    assert CR.knn(P.astype(np.float64), 5)[0] == 4 and CR.knn(P.astype(np.float64), 9)[0] == 9
    assert y["point_index"][7] == 4 and y["point_index"][16] == 10 and y["stats"]["spread"] == 8
    P, fpi, search = line_case(5, 1, [12], low_share=0.0)
    y = _check_reduce(_reduce_guarded(dev, _cf(P), fpi[None], search[None], cfg), 0, P, fpi, search, cfg, what="N=1")
    assert len(y["source_frame"]) == 5
    got = _reduce_guarded(dev, _cf(P), np.zeros((1, 0), np.int32), np.zeros((1, 0), np.float32), cfg)
    assert got["count"][0] == 0 and got["flags"][0] == 0
    P, fpi, search = line_case(6, 10, [0, 0, 0, 0, 30, 0, 0, 0, 0, 0], low_share=0.0)
    y = _check_reduce(_reduce_guarded(dev, _cf(P), fpi[None], search[None], cfg), 0, P, fpi, search, cfg, what="one")
    assert len(y["source_frame"]) == 9
    _check_reduce(_reduce_guarded(dev, _cf(P), fpi[None], search[None], cfg, cap=7), 0, P, fpi, search, cfg, cap=7,
                  what="overflow")
    for fpp, mnf, counts in ((1, 1, None), (1, 0, None), (255, 4, [0, 300, 0, 270, 1, 0])):
        c = CO.ContactReduceConfig(frame_per_point=fpp, max_neighbor_frame=mnf)
        P, fpi, search = line_case(7, 24 if counts is None else 6, counts, low_share=0.1)
        y = _check_reduce(_reduce_guarded(dev, _cf(P), fpi[None], search[None], c), 0, P, fpi, search, c, what=fpp)
        assert y["stats"]["over"] > 0
    # indices outside [0, count) count for nobody, and the walk ends
    P, fpi, search = line_case(8, 20, low_share=0.1)
    wild = fpi.copy()
    wild[::7] = ([-1, 20, 1 << 30, -(1 << 31)] * 50)[:len(wild[::7])]
    inside = (wild >= 0) & (wild < 15)
    got = _reduce_guarded(dev, _cf(P), wild[None], search[None], cfg, count=[15])
    y = CR.reduce(P[:15].astype(np.float64), np.where(inside, wild, -1), search)
    n = len(y["source_frame"])
    assert got["count"][0] == n and np.array_equal(got["source"][0, :n], y["source_frame"])
    assert np.array_equal(got["point"][0, :n], y["point_index"]) and (got["knn"][0, 15:] == -1).all()


# ---- batches, repeats, graphs, refusals ----

def _bits(r):
    from s4g_release_amd import contact_object as CO
    if isinstance(r, CO.ContactRefinement):
        return [r.counts, r.kept_i32, r.search_score, r.fail, r.kept_index, r.kept_count]
    if isinstance(r, CO.ContactReduction):
        return [r.source_frame, r.point_index, r.count, r.flags, r.neighbours]
    return [r.global_to_local, r.search_score, r.antipodal_score, r.frame_point_index, r.frame_count, r.flags]


def test_batch_invariance_and_repeats(dev):
    """Three objects of different point and frame counts in one padded batch against each alone, twice."""
    from s4g_release_amd import contact_object as CO
    sizes = ((900, 70), (257, 31), (1500, 120))
    M, F = max(s[0] for s in sizes), max(s[1] for s in sizes)
    xyz, g2l, search = np.zeros((3, 3, M), np.float32), np.zeros((3, F, 4, 4), np.float32), np.zeros((3, F), np.float32)
    xyz[:] = np.nan                                                        # padding that would show if it were read
    g2l[:] = np.nan
    search[:] = 999.0
    scenes = []
    for b, (m, f) in enumerate(sizes):
        P, G, s = lattice_scene(20 + b, m, f)
        xyz[b, :, :m], g2l[b, :f], search[b, :f] = P.T, G, s
        scenes.append((P, G, s))
    cfg = _edge_cfg()
    cnt = torch.tensor([s[0] for s in sizes], dtype=torch.int64, device=dev)
    fcnt = torch.tensor([s[1] for s in sizes], dtype=torch.int64, device=dev)
    runs = [CO.refine_contact_frames(_t(xyz, dev), _t(g2l, dev), _t(search, dev), cfg, cnt, fcnt) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(_bits(runs[0]), _bits(runs[1])))
    for b, (P, G, s) in enumerate(scenes):
        one = CO.refine_contact_frames(_t(_cf(P)[0], dev), _t(G, dev), _t(s, dev), cfg)
        assert one.unbatched and one.counts.shape[0] == 1
        f = len(G)
        for a, o in zip(_bits(runs[0])[:5], _bits(one)[:5]):
            assert torch.equal(a[b, :f], o[0]), b
        assert int(runs[0].kept_count[b]) == int(one.kept_count[0]) > 0
        assert (runs[0].fail[b, f:] == CO.REFINE_FAIL_FILTERED).all() and (runs[0].kept_index[b, f:] == -1).all()
    # the reduce stage
    rcfg = CO.ContactReduceConfig()
    cases = [line_case(30 + b, n, low_share=0.1) for b, n in enumerate((48, 17, 33))]
    N, F = 48, max(len(c[1]) for c in cases)
    xyz, fpi, search = np.zeros((3, 3, N), np.float32), np.full((3, F), 5, np.int32), np.full((3, F), 999.0, np.float32)
    for b, (P, i, s) in enumerate(cases):
        xyz[b, :, :len(P)], fpi[b, :len(i)], search[b, :len(s)] = P.T, i, s
    cnt = torch.tensor([len(c[0]) for c in cases], dtype=torch.int64, device=dev)
    fcnt = torch.tensor([len(c[1]) for c in cases], dtype=torch.int64, device=dev)
    runs = [CO.reduce_contact_frames(_t(xyz, dev), _t(fpi, dev), _t(search, dev), rcfg, cnt, fcnt) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(_bits(runs[0]), _bits(runs[1])))
    for b, (P, i, s) in enumerate(cases):
        one = CO.reduce_contact_frames(_t(_cf(P)[0], dev), _t(i, dev), _t(s, dev), rcfg)
        n = int(one.count[0])
        assert n == int(runs[0].count[b]) > 0 and one.unbatched
        assert torch.equal(runs[0].source_frame[b, :n], one.source_frame[0, :n])
        assert torch.equal(runs[0].point_index[b, :n], one.point_index[0, :n])
        assert (runs[0].source_frame[b, n:] == -1).all()
        assert torch.equal(runs[0].neighbours[b, :len(P)], one.neighbours[0])


def test_sync_free_and_graph_replay_of_the_chain(dev, stage1):
    from s4g_release_amd import contact_object as CO

    def run():
        return CO.reduce_contact_object(CO.refine_contact_object(stage1))

    eager = run()
    torch.cuda.synchronize(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
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
    assert all(torch.equal(a, b) for a, b in zip(_bits(eager), _bits(out)))
    assert int(out.frame_count[0]) > 1900


def test_refusals_leave_the_outputs_untouched(dev):
    from s4g_release_amd import _cabi, contact_object as CO
    P, G, search = lattice_scene(3, 64, 8)
    for kw in (dict(min_search_score=0), dict(min_search_score=1 << 24), dict(collision_threshold=-1)):
        cfg = CO.ContactRefineConfig(**kw)
        _refine_guarded(dev, _cf(P), G[None], search[None], cfg, expect_rc=_cabi.S4G_EINVAL)
    Pl, fpi, s = line_case(1, 16)
    for kw in (dict(frame_per_point=256), dict(frame_per_point=0), dict(max_neighbor_frame=6), dict(max_nn=8, min_rest=6)):
        cfg = CO.ContactReduceConfig(**kw)
        _reduce_guarded(dev, _cf(Pl), fpi[None], s[None], cfg, cap=16, expect_rc=_cabi.S4G_EINVAL)
    xyz, g2l, sc = _t(_cf(P), dev), _t(G[None], dev), _t(search[None], dev)
    with pytest.raises(ValueError):
        CO.refine_contact_frames(xyz, g2l, sc, CO.ContactRefineConfig(min_search_score=0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CO.refine_contact_frames(torch.from_numpy(_cf(P)), g2l, sc)
    with pytest.raises(RuntimeError, match="search_score"):
        CO.refine_contact_frames(xyz, g2l, sc[:, :5])
    with pytest.raises(RuntimeError, match="float32"):
        CO.refine_contact_frames(xyz, g2l.double(), sc)
    with pytest.raises(ValueError, match="min_rest"):
        CO.reduce_contact_frames(_t(_cf(Pl), dev), _t(fpi[None], dev), _t(s[None], dev),
                                 CO.ContactReduceConfig(max_nn=8, min_rest=6))
    with pytest.raises(ValueError, match="65536"):
        CO.reduce_contact_frames(torch.zeros((1, 3, CO.REDUCE_MAX_POINTS + 1), device=dev), _t(fpi[None], dev),
                                 _t(s[None], dev))
    with pytest.raises(RuntimeError, match="frame_point_index"):
        CO.reduce_contact_frames(_t(_cf(Pl), dev), _t(fpi[None], dev).float(), _t(s[None], dev))
