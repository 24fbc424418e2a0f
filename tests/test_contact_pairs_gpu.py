"""The contact model's per-object data on the device (`postprocess.contact_pairs`, `grade_contact_pairs`,
`label_contact_object`, `compose_contact_scene`; csrc/contact_pairs.hip) against the fixture the reference's own
`cache_contact_pair`, `_estimate_grasp_quality` and `get_frame_neighbor` produced (tests/golden/contact_pairs.npz) and
the float64 yardstick of tests/contact_pairs_ref.py (checked on the CPU by tests/test_contact_pairs_ref.py).

Tolerances.  Pairs, counts, validity and point indices exact, scores bit for bit, each on the rows the yardstick calls
decided (exact, for the counts) at the fixture's own eps0.  pair_score: the yardstick's double rounded to fp32 once;
the device forms the same double from the same fp32 inputs in the same order, and an fp32 rounding moves only where
the double sits within 1e-15 of a rounding boundary, so equality is asked to 1 ulp and counted bit for bit.
Frames: FRAME_TOL of the float64 yardstick.  An entry of global_to_local = L2LS[roll] @ T is a sum of three products
and (in the last column) one term more.  T is the double rounded once (2^-24 relative per entry, entries below 1 in
the rotation and below 0.5 m in the offset); the roll table is the reference's fp32 inverse of an fp32 matrix with
entries below 1, within 4 * 2^-24 of the exact inverse (tests/test_contact_pairs_ref.py pins 1e-6); each of the
seven operations rounds a partial sum below 2 by 2^-24 relative.  Together (3 * (1 + 4) + 7 * 2) * 2^-24 = 1.7e-6,
and FRAME_TOL = 2e-6.

The grading edge clouds sit on a 1 / 2048 m lattice, their pairs along the global x axis and the rolls at multiples of
90 degrees: every frame is axis-aligned, every local coordinate exact in fp32 up to the 0.078 m move-back, and no
bound is within 5e-5 m of a lattice value, so EVERY row is exact there (asserted)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import contact_pairs_ref as CP
from tests import golden_util as GU

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -559038737
FRAME_TOL = 2e-6
SWEEP, CHUNK = 1024, 1024                  # csrc/contact_pairs.hip: 256 lanes x CP_U, CP_CHUNK_POINTS
WG_PASS, GRID_X = 16, 256                  # CP_SLOTS, CP_GX
STEP = 1.0 / 2048


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


def _pairs_guarded(dev, xyz, nrm, count=None, max_pairs=None, cfg=None):
    """s4g_contact_pairs_f32 through the C ABI with every output inside a guarded buffer -> dict of numpy arrays."""
    from s4g_release_amd import _cabi, postprocess as PP
    from s4g_release_amd import functions as Fn
    cfg = cfg or PP.ContactPairConfig()
    B, _, N = xyz.shape
    if max_pairs is None:
        max_pairs = N * (N - 1) // 2
    d_x, d_n = _t(xyz, dev), _t(nrm, dev)
    d_c = None if count is None else _t(np.asarray(count, np.int64), dev)
    bufs = {k: _guarded(s, dev) for k, s in (("pairs", (B, max_pairs, 2)), ("score", (B, max_pairs)),
                                             ("count", (B, 2)), ("flags", (B,)))}
    nbytes = int(_cabi.lib().s4g_contact_pairs_workspace_bytes(B, N))
    ws = torch.full((nbytes + 2 * GUARD * 4,), 0x5A, dtype=torch.uint8, device=dev)
    rc = _cabi.lib().s4g_contact_pairs_f32(
        d_x.data_ptr(), d_n.data_ptr(), None if d_c is None else d_c.data_ptr(), B, N, max_pairs,
        float(cfg.max_distance), float(cfg.cos_threshold), bufs["pairs"][1].data_ptr() if max_pairs else None,
        bufs["score"][1].data_ptr() if max_pairs else None, bufs["count"][1].data_ptr(), bufs["flags"][1].data_ptr(),
        ws[GUARD * 4:].data_ptr(), nbytes, Fn._stream())
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    assert (ws[:GUARD * 4] == 0x5A).all() and (ws[GUARD * 4 + nbytes:] == 0x5A).all(), "guard of the workspace"
    return _read(bufs, floats=("score",), longs=("count",))


def _check_pairs(got, b, P, Nn, max_pairs=None, what=""):
    """Object b of a guarded result against the yardstick on the (N, 3) cloud P, Nn (the points that count)."""
    y = CP.pairs(P, Nn) if len(P) > 1 else {"row": np.zeros(0, int), "col": np.zeros(0, int), "score": np.zeros(0),
                                            "decided": np.zeros(0, bool), "near": np.zeros((2, 0), int)}
    assert y["decided"].all() and y["near"].shape[1] == 0, what          # (the edge clouds leave nothing undecided)
    K = len(y["row"])
    cap = got["pairs"].shape[1] if max_pairs is None else max_pairs
    n = min(K, cap)
    assert got["count"][b] == K, (what, got["count"][b], K)              # exact, also when the list does not fit
    assert got["flags"][b] == (1 if K > cap else 0), what
    assert np.array_equal(got["pairs"][b, :n, 0], y["row"][:n]) and np.array_equal(got["pairs"][b, :n, 1], y["col"][:n]), what
    assert np.array_equal(got["score"][b, :n], y["score"][:n].astype(np.float32)), what
    assert (got["pairs"][b, n:] == -1).all() and (got["score"][b, n:] == 0).all(), what
    return y


def _slab_cloud(seed, N, spread=0.012, lone_first=False):
    """Two facing planes 4 cm apart, normals along x: pairs across, none within a plane; lone_first: point 0 alone on
    its plane, so that row 0 has N - 1 candidates."""
    rng = np.random.default_rng(seed)
    side = rng.integers(0, 2, N) if not lone_first else np.r_[0, np.ones(N - 1, int)]
    P = np.stack([np.where(side == 0, -0.02, 0.02) + rng.uniform(-0.001, 0.001, N), rng.uniform(-spread, spread, N),
                  rng.uniform(-spread, spread, N)], 1)
    Nn = np.stack([np.where(side == 0, 1.0, -1.0), np.zeros(N), np.zeros(N)], 1) + rng.normal(0, 0.05, (N, 3))
    Nn /= np.linalg.norm(Nn, axis=1, keepdims=True)
    return P.astype(np.float32), Nn.astype(np.float32)


def _cf(a):
    """(N, 3) -> (1, 3, N) contiguous"""
    return np.ascontiguousarray(a.T[None])


# ---- pair enumeration ----

@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257])
def test_pairs_sizes(dev, N):
    P, Nn = _slab_cloud(N, N, spread=0.006 if N == 257 else 0.012, lone_first=N == 257)
    got = _pairs_guarded(dev, _cf(P), _cf(Nn), max_pairs=max(1, N * (N - 1) // 2))
    y = _check_pairs(got, 0, P.astype(np.float64), Nn.astype(np.float64), what="N=%d" % N)
    if N == 257:
        assert np.bincount(y["row"]).max() > 64                          # a row with more than one ballot of partners
    if N >= 63:
        assert len(y["row"]) > 0


def test_pairs_none_and_capacity(dev):
    P, Nn = _slab_cloud(5, 90)
    one = P.copy()
    one[:, 0] = -0.02                                                    # one plane: no pair
    got = _pairs_guarded(dev, _cf(one), _cf(Nn), max_pairs=50)
    _check_pairs(got, 0, one.astype(np.float64), Nn.astype(np.float64), what="zero pairs")
    K = len(CP.pairs(P.astype(np.float64), Nn.astype(np.float64))["row"])
    assert K > 100
    for cap in (K, K - 1):
        got = _pairs_guarded(dev, _cf(P), _cf(Nn), max_pairs=cap)
        _check_pairs(got, 0, P.astype(np.float64), Nn.astype(np.float64), what="max_pairs=%d of %d" % (cap, K))
        assert got["flags"][0] == (0 if cap == K else 1)


def test_pairs_nan_count_and_batch(dev):
    big, nbig = _slab_cloud(7, 150)
    small, nsmall = _slab_cloud(8, 70)
    holed = big.copy()
    holed[11, 1] = np.nan
    holed[40] = np.inf
    # a point that is not finite pairs with nothing: the same list as with the point moved far away
    away = holed.copy().astype(np.float64)
    away[[11, 40]] = [[5.0, 5.0, 5.0], [-5.0, 5.0, 5.0]]
    got = _pairs_guarded(dev, _cf(holed), _cf(nbig))
    _check_pairs(got, 0, away, nbig.astype(np.float64), what="NaN point")
    # count shorter than N, and two objects of different size in one batch against each alone
    xyz = np.zeros((2, 3, 150), np.float32)
    nrm = np.zeros((2, 3, 150), np.float32)
    xyz[0], nrm[0] = big.T, nbig.T
    xyz[1, :, :70], nrm[1, :, :70] = small.T, nsmall.T
    xyz[1, :, 70:] = np.nan                                              # (never read as points)
    cap = 150 * 149 // 2
    both = _pairs_guarded(dev, xyz, nrm, count=[150, 70], max_pairs=cap)
    _check_pairs(both, 0, big.astype(np.float64), nbig.astype(np.float64), what="batch 0")
    _check_pairs(both, 1, small.astype(np.float64), nsmall.astype(np.float64), what="batch 1")
    alone = _pairs_guarded(dev, _cf(small), _cf(nsmall), max_pairs=cap)
    for k in ("pairs", "score", "count", "flags"):
        assert np.array_equal(both[k][1], alone[k][0]), k
    short = _pairs_guarded(dev, _cf(big), _cf(nbig), count=[99], max_pairs=cap)
    _check_pairs(short, 0, big[:99].astype(np.float64), nbig[:99].astype(np.float64), what="count 99 of 150")


# ---- pair grading on lattice clouds ----

def _edge_cfg(**over):
    from s4g_release_amd import postprocess as PP
    kw = dict(theta_search=(0, 90, 180, 270), min_points=3)
    kw.update(over)
    return PP.ContactPairConfig(**kw)


def _grade_guarded(dev, xyz, pairs, cfg, pair_score=None, pair_count=None, count=None, max_frames=None):
    """s4g_contact_pair_grade_f32 through the C ABI with every output inside a guarded buffer -> dict of numpy arrays."""
    from s4g_release_amd import _cabi
    from s4g_release_amd import functions as Fn
    B, _, N = xyz.shape
    P = pairs.shape[1]
    T, W = len(cfg.theta_search), len(cfg.width_shift)
    F = P * T if max_frames is None else max_frames
    d_x, d_p = _t(xyz, dev), _t(pairs.astype(np.int32), dev)
    d_s = None if pair_score is None else _t(pair_score.astype(np.float32), dev)
    d_pc = None if pair_count is None else _t(np.asarray(pair_count, np.int64), dev)
    d_c = None if count is None else _t(np.asarray(count, np.int64), dev)
    bufs = {k: _guarded(s, dev) for k, s in (
        ("counts", (B, P, T, W, 3)), ("close_plane", (B, P)), ("score", (B, P, T)), ("valid", (B, P, T)),
        ("fail", (B, P)), ("g2l", (B, F, 4, 4)), ("search", (B, F)), ("antipodal", (B, F)), ("source", (B, F)),
        ("index", (B, F)), ("frame_count", (B, 2)), ("flags", (B,)))}
    once = lambda v: float(np.float32(v))                                            # noqa: E731
    params = (ctypes.c_float * 5)(once(cfg.half_bottom_width), once(cfg.half_bottom_space),
                                  once(cfg.back_collision_margin), once(cfg.bottom_length), once(cfg.finger_length))
    gates = (ctypes.c_double * 3)(float(cfg.min_points), float(cfg.back_threshold), float(cfg.finger_threshold))
    tables = cfg.tables().to(dev)
    nbytes = int(_cabi.lib().s4g_contact_pair_grade_workspace_bytes(B, N, P, T, W))
    ws = torch.full((nbytes + 2 * GUARD * 4,), 0x5A, dtype=torch.uint8, device=dev)
    ptr = lambda k: bufs[k][1].data_ptr() if bufs[k][1].numel() else None            # noqa: E731
    opt = lambda t: None if t is None else t.data_ptr()                              # noqa: E731
    rc = _cabi.lib().s4g_contact_pair_grade_f32(
        d_x.data_ptr(), opt(d_c), d_p.data_ptr() if P else None, opt(d_s), opt(d_pc), B, N, P, T, W, params, gates,
        tables.data_ptr(), F, ptr("counts"), ptr("close_plane"), ptr("score"), ptr("valid"), ptr("fail"), ptr("g2l"),
        ptr("search"), ptr("antipodal"), ptr("source"), ptr("index"), ptr("frame_count"), ptr("flags"),
        ws[GUARD * 4:].data_ptr(), nbytes, Fn._stream())
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    assert (ws[:GUARD * 4] == 0x5A).all() and (ws[GUARD * 4 + nbytes:] == 0x5A).all(), "guard of the workspace"
    return _read(bufs, floats=("score", "g2l", "search", "antipodal"), longs=("frame_count",))


def _yard(P, row, col, cfg, eps0):
    """The yardstick over the DISTINCT pairs of a list that may repeat them -> (grade dict, the index of each row)."""
    key = np.asarray(row, np.int64) * (len(P) + 1) + np.asarray(col, np.int64)
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    g = CP.grade(P, np.asarray(row)[first], np.asarray(col)[first], eps0, theta=cfg.theta_search,
                 shifts=cfg.width_shift, min_points=cfg.min_points, back_threshold=cfg.back_threshold,
                 finger_threshold=cfg.finger_threshold)
    return g, inverse


def _check_grade(got, b, P, row, col, cfg, eps0, pair_score=None, max_frames=None, all_exact=True, what=""):
    """Object b of a guarded result against the yardstick on the (N, 3) float64 cloud P and the pair list."""
    g, at = _yard(P, row, col, cfg, eps0)
    K, T = len(row), len(cfg.theta_search)
    d, e = g["decided"][at], g["exact"][at]
    if all_exact:
        assert e[g["finite"][at]].all(), what
    fin = g["finite"][at]
    assert np.array_equal((got["fail"][b, :K] & 1) != 0, ~fin), what
    assert np.array_equal(got["valid"][b, :K][d] != 0, g["valid"][at][d]), what
    assert np.array_equal(got["score"][b, :K][d].view(np.int32), g["score"][at][d].view(np.int32)), what
    assert np.array_equal(got["counts"][b, :K][e], g["counts"][at][e]), what
    pe = e.all(1)
    assert np.array_equal(got["close_plane"][b, :K][pe], g["close_plane"][at][pe]), what
    assert np.array_equal((got["fail"][b, :K][pe & fin] & 2) != 0, g["close_plane"][at][pe & fin] < cfg.min_points), what
    for k in ("counts", "close_plane", "score", "valid", "fail"):
        assert (got[k][b, K:] == 0).all(), (what, k)                       # rows at or past pair_count
    # the frame list: the device's own valid rows in ascending pair * T + roll
    src = np.flatnonzero(got["valid"][b].reshape(-1))
    F = got["source"].shape[1] if max_frames is None else max_frames
    n = min(len(src), F)
    assert got["frame_count"][b] == len(src) and got["flags"][b] == (2 if len(src) > F else 0), what
    assert np.array_equal(got["source"][b, :n], src[:n]) and (got["source"][b, n:] == -1).all(), what
    assert (got["index"][b, n:] == -1).all() and (got["g2l"][b, n:] == 0).all() and (got["search"][b, n:] == 0).all(), what
    pair, roll = src[:n] // T, src[:n] % T
    assert np.array_equal(got["search"][b, :n].view(np.int32), got["score"][b].reshape(-1)[src[:n]].view(np.int32)), what
    if pair_score is not None:
        assert np.array_equal(got["antipodal"][b, :n], pair_score[pair].astype(np.float32)), what
    L = CP.local_to_local_search(cfg.theta_search)
    want = L[roll] @ g["T"][at][pair]
    assert n == 0 or np.abs(got["g2l"][b, :n] - want).max() < FRAME_TOL, what
    idx, sure = CP.nearest(P, want)
    assert np.array_equal(got["index"][b, :n][sure], idx[sure]), what
    return g, at, n


def _lattice_cloud(seed, N, mates):
    """N lattice points in a slab a gripper can close on; the first `mates` points have a mate (points mates..2 mates)
    with the same y and z: pairs along the global x axis."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.integers(-20, 20, N), rng.integers(-30, 20, N), rng.integers(-60, 60, N)], 1).astype(np.float64)
    for m in range(mates):
        p[mates + m, 1:] = p[m, 1:]
        p[mates + m, 0] = p[m, 0] + rng.integers(8, 40)
    return p * STEP


def _x_pairs(mates, K):
    k = np.arange(K) % max(mates, 1)
    return k, k + mates


@pytest.mark.parametrize("N", [1, 7, 49, 50, SWEEP - 1, SWEEP, SWEEP + 1])
def test_grade_cloud_sizes(dev, fx, N):
    cfg = _edge_cfg()
    mates = min(N // 2, 6)
    P = _lattice_cloud(N, N, mates)
    row, col = _x_pairs(mates, 9)                                          # N = 1: the pair (0, 0), degenerate
    got = _grade_guarded(dev, _cf(P.astype(np.float32)), np.stack([row, col], 1)[None], cfg)
    g, at, n = _check_grade(got, 0, P, row, col, cfg, float(fx["eps0"][0]), what="N=%d" % N)
    if N >= SWEEP - 1:
        assert n > 0                                                       # valid frames, not only refusals
    if N == 1:
        assert (got["fail"][0] == 1).all() and n == 0


@pytest.mark.parametrize("K", [WG_PASS * GRID_X - 1, WG_PASS * GRID_X, WG_PASS * GRID_X + 1, GRID_X - 1, GRID_X,
                               GRID_X + 1])
def test_grade_pair_counts(dev, fx, K):
    cfg = _edge_cfg()
    P = _lattice_cloud(3, 300, 37)
    row, col = _x_pairs(37, K)
    score = np.linspace(0.95, 1.0, K).astype(np.float32)
    got = _grade_guarded(dev, _cf(P.astype(np.float32)), np.stack([row, col], 1)[None], cfg, pair_score=score)
    g, at, n = _check_grade(got, 0, P, row, col, cfg, float(fx["eps0"][0]), pair_score=score, what="K=%d" % K)
    assert n > K // 8


def test_grade_frame_capacity_pair_count_and_batch(dev, fx):
    cfg = _edge_cfg()
    P = _lattice_cloud(4, 300, 37)
    row, col = _x_pairs(37, 60)
    prs = np.stack([row, col], 1)[None]
    full = _grade_guarded(dev, _cf(P.astype(np.float32)), prs, cfg)
    count = int(full["frame_count"][0])
    assert count > 8
    for cap in (count, count - 1):
        got = _grade_guarded(dev, _cf(P.astype(np.float32)), prs, cfg, max_frames=cap)
        _check_grade(got, 0, P, row, col, cfg, float(fx["eps0"][0]), max_frames=cap, what="max_frames=%d" % cap)
        assert got["flags"][0] == (0 if cap == count else 2) and got["frame_count"][0] == count
    # two objects of different size and different pair counts in one batch against each alone
    Q = _lattice_cloud(5, 120, 20)
    qrow, qcol = _x_pairs(20, 25)
    xyz = np.zeros((2, 3, 300), np.float32)
    xyz[0] = P.T
    xyz[1, :, :120] = Q.T
    xyz[1, :, 120:] = np.nan
    two = np.full((2, 60, 2), -1, np.int32)
    two[0] = prs[0]
    two[1, :25] = np.stack([qrow, qcol], 1)
    both = _grade_guarded(dev, xyz, two, cfg, pair_count=[60, 25], count=[300, 120])
    _check_grade(both, 0, P, row, col, cfg, float(fx["eps0"][0]), what="batch 0")
    _check_grade(both, 1, Q, qrow, qcol, cfg, float(fx["eps0"][0]), what="batch 1")
    alone = _grade_guarded(dev, _cf(Q.astype(np.float32)), two[1:, :25], cfg)
    for k in ("counts", "close_plane", "score", "valid", "fail"):
        assert np.array_equal(both[k][1, :25], alone[k][0]), k
    n = int(alone["frame_count"][0])
    assert n == both["frame_count"][1]
    for k in ("g2l", "search", "source", "index"):
        assert np.array_equal(both[k][1, :n], alone[k][0, :n]), k


def _hand_cloud(centre, minus, plus, behind):
    """The pair (-0.02, 0, 0), (0.02, 0, 0): local x = global y, local y = global x, local z = -global z, and with the
    one roll of 0 degrees sx = y + 0.078, sz = -z.  `centre`, `minus`, `plus` points in the close region of the shift
    0, -0.015, +0.015 (the two pair points count for the centre); `behind`: a point behind the palm in the centre slab."""
    pts = [(-0.02, 0.0, 0.0), (0.02, 0.0, 0.0)]
    pts += [(0.001 * (k - 4), -0.01, 0.0005 * (k % 3)) for k in range(centre - 2)]
    pts += [(0.001 * (k - 4), -0.02, 0.02) for k in range(minus)]          # sz = -0.02: in (-0.027, -0.003) only
    pts += [(0.001 * (k - 4), -0.03, -0.02) for k in range(plus)]
    if behind:
        pts.append((0.0, -0.1, 0.0))                                       # sx = -0.022: behind the palm, sz = 0
    return np.array(pts, np.float64)


@pytest.mark.parametrize("case,centre,minus,plus,behind,valid,score", [
    ("control", 9, 6, 6, False, True, 7.0),
    ("last shift skipped by a collision", 9, 6, 6, True, False, 0.0),
    ("last shift clear but short", 2, 6, 6, False, False, 0.0),
    ("sum short, centre above", 5, 0, 0, False, False, 0.0)])
def test_grade_constructed_gates(dev, fx, case, centre, minus, plus, behind, valid, score):
    cfg = _edge_cfg(theta_search=(0,))
    P = _hand_cloud(centre, minus, plus, behind)
    P = np.float32(P).astype(np.float64)
    row, col = np.array([0]), np.array([1])
    got = _grade_guarded(dev, _cf(P.astype(np.float32)), np.stack([row, col], 1)[None], cfg)
    g, at, n = _check_grade(got, 0, P, row, col, cfg, float(fx["eps0"][0]), what=case)
    c = got["counts"][0, 0, 0]                                             # (W, 3)
    assert c[:, 2].tolist() == [minus, plus, centre] and c[2, 0] == (1 if behind else 0) and c[:2, 0].tolist() == [0, 0]
    assert bool(got["valid"][0, 0, 0]) == valid and got["score"][0, 0, 0] == np.float32(score), case
    if case == "sum short, centre above":
        assert np.float32(centre) / np.float32(3) < cfg.min_points <= centre


def test_grade_degenerate_pairs(dev, fx):
    cfg = _edge_cfg()
    P = _lattice_cloud(6, 200, 10)
    P[20] = P[21] + [0, 16 * STEP, 0]                                      # a pair along e_y: x = e_y - (e_y . y) y = 0
    row, col = np.array([0, 20, 5, 5, 1]), np.array([10, 21, 5, 15, 11])   # ..., coincident, ...
    got = _grade_guarded(dev, _cf(P.astype(np.float32)), np.stack([row, col], 1)[None], cfg)
    _check_grade(got, 0, P, row, col, cfg, float(fx["eps0"][0]), what="degenerate")
    assert (got["fail"][0] & 1).tolist() == [0, 1, 1, 0, 0]
    assert (got["valid"][0, 1:3] == 0).all() and (got["counts"][0, 1:3] == 0).all()
    bad = np.array([[0, 200], [-1, 3]])                                    # an index outside the object
    got = _grade_guarded(dev, _cf(P.astype(np.float32)), bad[None], cfg)
    assert (got["fail"][0] == 4).all() and got["frame_count"][0] == 0 and (got["valid"][0] == 0).all()


# ---- the fixture through label_contact_object ----

@pytest.fixture(scope="module")
def fx():
    g = GU.load("contact_pairs.npz")
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def yard(fx):
    """The yardstick's grade of the fixture's strided subset, computed once.  (The pair list is compared with the
    reference's own: tests/test_contact_pairs_ref.py pins that the yardstick gives the same list, none undecided.)"""
    sub = fx["subset"]
    return CP.grade(fx["points"].astype(np.float64), fx["pair_row"][sub], fx["pair_col"][sub], float(fx["eps0"][0]))


def _label_fixture(dev, fx, B=1, **kw):
    from s4g_release_amd import postprocess as PP
    xyz = _t(np.stack([fx["points"].T] * B), dev)
    nrm = _t(np.stack([fx["normals"].T] * B), dev)
    K = len(fx["pair_row"])
    return PP.label_contact_object(xyz, nrm, max_pairs=kw.pop("max_pairs", K), max_frames=kw.pop("max_frames", 5 * K), **kw)


@pytest.fixture(scope="module")
def eager(dev, fx):
    out = _label_fixture(dev, fx)
    torch.cuda.synchronize(dev)
    return out


def _bits(o):
    return [o.global_to_local.view(torch.int32), o.search_score.view(torch.int32), o.antipodal_score.view(torch.int32),
            o.frame_point_index, o.frame_count, o.flags, o.pairs.pairs, o.pairs.score.view(torch.int32), o.pairs.count,
            o.grades.counts, o.grades.close_plane, o.grades.score.view(torch.int32), o.grades.valid_i32, o.grades.fail,
            o.grades.frame_source]


def test_fixture_pairs(fx, eager):
    K = len(fx["pair_row"])
    assert int(eager.pairs.count[0]) == K and int(eager.flags[0]) == 0
    got = eager.pairs.pairs[0].cpu().numpy()
    assert np.array_equal(got[:, 0], fx["pair_row"]) and np.array_equal(got[:, 1], fx["pair_col"])
    score = eager.pairs.score[0].cpu().numpy()
    want = fx["pair_score"].astype(np.float32)
    ulp = np.abs(score.view(np.int32) - want.view(np.int32))
    print("pair_score: %d of %d differ from the reference's double rounded once, by at most %d ulp"
          % ((ulp > 0).sum(), K, ulp.max()))
    assert ulp.max() <= 1 and (ulp > 0).sum() == 0


def test_fixture_grading_and_frames(fx, yard, eager):
    g = yard
    sub = fx["subset"].astype(np.int64)
    T = len(CP.THETA_SEARCH)
    G = eager.grades
    d, e = g["decided"], g["exact"]
    valid = G.valid_i32[0].cpu().numpy()[sub] != 0
    score = G.score[0].cpu().numpy()[sub]
    ref_valid = np.zeros_like(g["valid"])
    ref_valid[fx["frame_pair"], fx["frame_roll"]] = True
    ref_score = np.zeros_like(g["score"])
    ref_score[fx["frame_pair"], fx["frame_roll"]] = fx["search_score"]
    assert np.array_equal(valid[d], ref_valid[d])                          # the reference itself
    assert np.array_equal(score[d].view(np.int32), ref_score[d].view(np.int32))
    assert np.array_equal(G.counts[0].cpu().numpy()[sub][e], g["counts"][e])
    pe = e.all(1)
    assert np.array_equal(G.close_plane[0].cpu().numpy()[sub][pe], g["close_plane"][pe])
    assert (G.fail[0].cpu().numpy() & 5 == 0).all()
    # the frame list
    n = int(eager.frame_count[0])
    allv = G.valid_i32[0].cpu().numpy().reshape(-1)
    src = G.frame_source[0].cpu().numpy()
    assert n == int((allv != 0).sum()) and n <= src.shape[0] and np.array_equal(src[:n], np.flatnonzero(allv))
    assert (src[n:] == -1).all() and (eager.frame_point_index[0, n:] == -1).all()
    where = {int(s): f for f, s in enumerate(src[:n])}
    g2l = eager.global_to_local[0].cpu().numpy()
    fpi = eager.frame_point_index[0].cpu().numpy()
    search = eager.search_score[0].cpu().numpy()
    anti = eager.antipodal_score[0].cpu().numpy()
    fr = CP.frames(g)
    idx, sure = CP.nearest(fx["points"].astype(np.float64), fr["global_to_local"])
    at = {(p, t): i for i, (p, t) in enumerate(zip(fr["pair"].tolist(), fr["roll"].tolist()))}
    compared = worst = 0
    for f, (p, t) in enumerate(zip(fx["frame_pair"].tolist(), fx["frame_roll"].tolist())):
        if not d[p, t]:
            continue
        row = where[int(sub[p]) * T + t]
        i = at[(p, t)]
        worst = max(worst, np.abs(g2l[row] - fr["global_to_local"][i]).max())
        assert search[row] == fx["search_score"][f]
        assert anti[row] == np.float32(fx["antipodal_score"][f])
        if sure[i]:
            compared += 1
            assert fpi[row] == fx["frame_point_index"][f] == idx[i]
    print("frames: worst distance from float64 %.3g (bound %.3g); %d point indices compared" % (worst, FRAME_TOL, compared))
    assert worst < FRAME_TOL and compared >= 1000


def test_fixture_dump_matches_the_reference_dictionary(fx, eager):
    dump = eager.dump(0)
    assert sorted(dump) == ["antipodal_score", "cloud", "frame_point_index", "global_to_local", "normal", "search_score"]
    n = int(eager.frame_count[0])
    assert dump["cloud"].shape == (len(fx["points"]), 3) and np.array_equal(dump["cloud"], fx["points"])
    assert dump["global_to_local"].shape == (n, 4, 4) and dump["frame_point_index"].shape == (n,)


# ---- invariance ----

def test_run_to_run_batch_graph_and_no_sync(dev, fx, eager):
    again = _label_fixture(dev, fx)
    assert all(torch.equal(a, b) for a, b in zip(_bits(eager), _bits(again)))
    # the same bits alone and in a batch, next to a shorter object
    from s4g_release_amd import postprocess as PP
    K = len(fx["pair_row"])
    xyz = _t(np.stack([fx["points"].T] * 2), dev).clone()
    nrm = _t(np.stack([fx["normals"].T] * 2), dev)
    cnt = torch.tensor([1000, xyz.shape[2]], dtype=torch.int64, device=dev)
    two = PP.label_contact_object(xyz, nrm, count=cnt, max_pairs=K, max_frames=5 * K)
    for a, b in zip(_bits(eager), _bits(two)):
        assert torch.equal(a[0], b[1])
    assert 0 < int(two.pairs.count[0]) < K
    # no host synchronisation, and the same bits under a captured graph
    torch.cuda.synchronize(dev)
    one_xyz, one_nrm = xyz[:1].contiguous(), nrm[:1].contiguous()
    torch.cuda.synchronize(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        PP.label_contact_object(one_xyz, one_nrm, max_pairs=K, max_frames=5 * K)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    run = lambda: PP.label_contact_object(one_xyz, one_nrm, max_pairs=K, max_frames=5 * K)      # noqa: E731
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for _ in range(2):
        for t in _bits(out):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        assert all(torch.equal(a, b) for a, b in zip(_bits(eager), _bits(out)))


def test_cpu_tensors_and_unbatched(dev, fx):
    from s4g_release_amd import postprocess as PP
    P, Nn = _slab_cloud(9, 80)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.label_contact_object(torch.from_numpy(P.T.copy()), torch.from_numpy(Nn.T.copy()))
    one = PP.label_contact_object(_t(P.T.copy(), dev), _t(Nn.T.copy(), dev))
    assert one.unbatched and one.global_to_local.dim() == 4 and one.global_to_local.shape[0] == 1
    y = CP.pairs(P.astype(np.float64), Nn.astype(np.float64))
    assert int(one.pairs.count[0]) == len(y["row"])


# ---- end to end: two objects through compose_contact_scene into grade_contact_frames ----

def test_compose_scene_into_grade_contact_frames(dev, fx):
    from s4g_release_amd import postprocess as PP
    cfg = PP.ContactPairConfig(min_points=10)
    n1, n2 = 900, 700
    a = PP.label_contact_object(_t(fx["points"][:n1].T.copy(), dev), _t(fx["normals"][:n1].T.copy(), dev), cfg)
    b = PP.label_contact_object(_t(fx["points"][n1:n1 + n2].T.copy(), dev), _t(fx["normals"][n1:n1 + n2].T.copy(), dev), cfg)
    poses = [(0.1, -0.05, 0.9, 1.0, 0.0, 0.0, 0.0), (-0.1, 0.08, 0.95, np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5))]
    scene = PP.compose_contact_scene([a, b], poses, labels=[3, 8])
    f1, f2 = int(a.frame_count[0]), int(b.frame_count[0])
    assert f1 > 0 and f2 > 0 and int(a.flags[0]) == 0 and int(b.flags[0]) == 0
    assert tuple(scene.points.shape) == (3, n1 + n2) and tuple(scene.global_to_local.shape) == (f1 + f2, 4, 4)
    assert tuple(scene.frame_point_index.shape) == (f1 + f2,) and scene.frame_point_index.dtype == torch.int32
    # a numpy restatement of generate_single_scene (:57-100)
    want_p, want_g, want_i, start = [], [], [], 0
    for obj, pose, n in ((a, poses[0], n1), (b, poses[1], n2)):
        mat = np.eye(4)
        mat[:3, :3] = PP.quaternion_matrix(pose[3:]).numpy()
        mat[:3, 3] = pose[:3]
        d = obj.dump(0)
        homo = np.concatenate([d["cloud"].astype(np.float64), np.ones((n, 1))], 1).T
        want_p.append((mat @ homo)[:3])
        want_g.append(d["global_to_local"].astype(np.float64) @ np.linalg.inv(mat))
        want_i.append(d["frame_point_index"] + start)
        start += n
    assert np.abs(scene.points.cpu().numpy() - np.concatenate(want_p, 1)).max() < 1e-6
    assert np.abs(scene.global_to_local.cpu().numpy() - np.concatenate(want_g)).max() < 1e-5
    assert np.array_equal(scene.frame_point_index.cpu().numpy(), np.concatenate(want_i))
    assert np.array_equal(scene.labels.cpu().numpy(), np.r_[np.full(n1, 3), np.full(n2, 8)])
    assert (scene.frame_point_index[f1:] >= n1).all() and (scene.frame_point_index[:f1] < n1).all()
    search = PP.grade_contact_frames(scene.global_to_local, scene.points, scene.labels)
    assert tuple(search.valid_i32.shape) == (1, f1 + f2) and search.unbatched
