"""GPU tests of `render_views` (csrc/render_views.hip) against the float64 numpy yardstick (tests/render_ref.py) and
its committed fixture (tests/golden/render_views.npz).

The C entry is called with every input inside a NaN-filled buffer and every output and the workspace inside a poisoned
buffer with guard bytes on both sides, checked after the call.  Scenes of the EXACT FAMILY (axis-aligned cameras,
dyadic vertices and centres, power-of-two focal lengths: every product of the hit test is exact in double) are
compared bit for bit on every pixel and every output; the fixture's views, where the two sides may round differently,
on the yardstick's decided pixels and within one fp32 rounding of the stored range.

Measured on the fixture (MI355X; printed by test_fixture_views, copied to profiles/r31_render_views.md): see there."""
import os
import re

import numpy as np
import pytest
import torch

from tests import render_ref as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256                # bytes on both sides of every output and of the workspace
POISON = 0xA5
PAD = 64                   # NaN elements on both sides of every input
EINVAL, EWORKSPACE = -1, -2
OUTPUTS = ("range", "triangle", "points", "noisy", "pixel", "count", "workspace")


def _const(name):
    src = open(os.path.join(ROOT, "s4g_release_amd", "csrc", "render_views.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


TILE, CHUNK, CAP, SEG = _const("RV_TILE"), _const("RV_CHUNK"), _const("RV_CAP"), _const("RV_SEG")


@pytest.fixture(scope="module")
def lib():
    from s4g_release_amd import _cabi
    return _cabi.lib()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "render_views.npz")) as z:
        return {k: z[k] for k in z.files}


def _stream():
    from s4g_release_amd import functions
    return functions._stream()


class _Guarded:
    def __init__(self, dev):
        self.dev, self.bufs = dev, {}

    def add(self, name, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.uint8, device=self.dev)
        self.bufs[name] = (buf, buf[GUARD:GUARD + n].view(dtype).view(shape), n)
        return self.bufs[name][1].data_ptr()

    def read(self):
        torch.cuda.synchronize(self.dev)
        out = {}
        for k, (buf, view, n) in self.bufs.items():
            assert (buf[:GUARD] == POISON).all() and (buf[GUARD + n:] == POISON).all(), "guard of %s" % k
            out[k] = view.cpu().numpy()
        return out

    def untouched(self):
        torch.cuda.synchronize(self.dev)
        return all(bool((b[0] == POISON).all()) for b in self.bufs.values())


def _padded(a, dtype, dev):
    """a inside a NaN-filled device buffer -> (the view, its owner)."""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.size + 2 * PAD,), float("nan"), dtype=dtype, device=dev)
    buf[PAD:PAD + a.size] = torch.from_numpy(a).to(dev).reshape(-1)
    return buf[PAD:PAD + a.size], buf


def _call(lib, dev, tri, cams, K, count=None, noise=None, expect=0, told=None, ws_short=0, null_ws=False):
    """s4g_render_views_f32 through the C ABI.  tri (B, T, 3, 3) fp32, cams (B, V, 12) float64, noise (B, V, P) float64
    or None -> dict of numpy outputs (expect == 0) or whether everything was left untouched (a refusal).  told: the
    values the entry is told where they are not the buffers' (a dict over B V T H W fx fy cx cy)."""
    tri = np.asarray(tri, np.float32)
    cams = np.asarray(cams, np.float64)
    B, T = tri.shape[:2]
    V = cams.shape[1]
    P = K.H * K.W
    x, _x = _padded(tri.reshape(-1) if T else np.zeros(1, np.float32), torch.float32, dev)
    cm, _cm = _padded(cams.reshape(-1), torch.float64, dev)
    cnt = None if count is None else torch.from_numpy(np.asarray(count, np.int32)).to(dev)
    nz = None
    if noise is not None:
        nz, _nz = _padded(np.asarray(noise, np.float64).reshape(-1), torch.float64, dev)
    a = dict(B=B, V=V, T=T, H=K.H, W=K.W, fx=K.fx, fy=K.fy, cx=K.cx, cy=K.cy)
    a.update(told or {})
    g = _Guarded(dev)
    p_range = g.add("range", (B, V, P), torch.float32)
    p_tri = g.add("triangle", (B, V, P), torch.int32)
    p_pts = g.add("points", (B, V, 3, P), torch.float32)
    p_nsy = g.add("noisy", (B, V, 3, P), torch.float32)
    p_pix = g.add("pixel", (B, V, P), torch.int32)
    p_cnt = g.add("count", (B, V), torch.int32)
    nbytes = int(lib.s4g_render_views_workspace_bytes(B, V, T, K.H, K.W))
    assert nbytes > 0
    p_ws = g.add("workspace", (nbytes,), torch.uint8)
    with torch.cuda.device(dev):
        rc = lib.s4g_render_views_f32(x.data_ptr(), None if cnt is None else cnt.data_ptr(), cm.data_ptr(), a["B"],
                                      a["V"], a["T"], a["fx"], a["fy"], a["cx"], a["cy"], K.max_depth, a["H"], a["W"],
                                      None if nz is None else nz.data_ptr(), p_range, p_tri, p_pts, p_nsy, p_pix, p_cnt,
                                      None if null_ws else p_ws, 0 if null_ws else nbytes - ws_short, _stream())
    assert rc == expect, rc
    if expect != 0:
        return g.untouched()
    out = g.read()
    if noise is None:
        assert (g.bufs["noisy"][0] == POISON).all()                    # not touched without multipliers
        out["noisy"] = None
    del out["workspace"]
    return out


def _ref(tri, cams, K, count=None, noise=None):
    """The yardstick over a batch -> (the dict `_call` returns, decided (B, V, P))."""
    tri = np.asarray(tri, np.float32)
    cams = np.asarray(cams, np.float64)
    B, V, P = tri.shape[0], cams.shape[1], K.H * K.W
    out = {"range": np.zeros((B, V, P), np.float32), "triangle": np.zeros((B, V, P), np.int32),
           "points": np.zeros((B, V, 3, P), np.float32), "noisy": None if noise is None else np.zeros((B, V, 3, P), np.float32),
           "pixel": np.zeros((B, V, P), np.int32), "count": np.zeros((B, V), np.int32)}
    decided = np.zeros((B, V, P), bool)
    for b in range(B):
        for v in range(V):
            R, c = cams[b, v, :9].reshape(3, 3), cams[b, v, 9:]
            res = RR.render_ref(tri[b], R, c, K, noise=None if noise is None else noise[b, v],
                                tri_count=None if count is None else count[b])
            pts, nsy, pix, k = RR.compact(res, P)
            out["range"][b, v], out["triangle"][b, v], out["points"][b, v] = res.range, res.triangle, pts
            out["pixel"][b, v], out["count"][b, v] = pix, k
            if noise is not None:
                out["noisy"][b, v] = nsy
            decided[b, v] = res.decided
    return out, decided


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_same(got, want, what=""):
    for k in ("triangle", "range", "count", "pixel", "points", "noisy"):
        if want[k] is None:
            assert got[k] is None, (what, k)
            continue
        if not _bits_equal(got[k], want[k]):
            a, b = got[k], want[k]
            bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
            raise AssertionError("%s: %s differs at %s: got %s, want %s" % (
                what, k, bad[:4].tolist(), [a[tuple(i)] for i in bad[:4]], [b[tuple(i)] for i in bad[:4]]))


def _check_compaction(out, K):
    """The compact outputs against the dense ones of the same call: ascending pixel order equal to the dense mask."""
    B, V, P = out["range"].shape
    pix_all = np.arange(P)
    rx, ry = (pix_all % K.W + 0.5 - K.cx) / K.fx, (pix_all // K.W + 0.5 - K.cy) / K.fy
    dz = 1.0 / np.sqrt(rx * rx + ry * ry + 1.0)
    for b in range(B):
        for v in range(V):
            with np.errstate(invalid="ignore"):
                mask = (out["triangle"][b, v] >= 0) & (out["range"][b, v].astype(np.float64) * dz < K.max_depth)
            k = int(out["count"][b, v])
            assert k == int(mask.sum())
            assert np.array_equal(out["pixel"][b, v, :k], np.nonzero(mask)[0])
            assert (out["pixel"][b, v, k:] == -1).all()
            for name in ("points", "noisy"):
                if out[name] is not None:
                    assert np.isfinite(out[name][b, v, :, :k]).all() and np.isnan(out[name][b, v, :, k:]).all()
            assert np.array_equal(np.isinf(out["range"][b, v]), out["triangle"][b, v] < 0)


# ---- the exact family -------------------------------------------------------------------------------------------------

EYE = RR.cam12(np.eye(3), np.zeros(3))
TURNED_R = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
TURNED_C = np.array([0.5, -0.25, 2.0])
TURNED = RR.cam12(TURNED_R, TURNED_C)


def _K(W, H, fx=8.0, max_depth=5.0, cx=None, cy=None):
    return RR.Intrinsics(fx, fx, W / 2.0 if cx is None else cx, H / 2.0 if cy is None else cy, max_depth, H, W)


def _px(K, x, y, depth):
    """The camera-frame point (fp32-exact for dyadic input) that projects to pixel coordinates (x, y) at `depth`."""
    return [(x - K.cx) / K.fx * depth, (y - K.cy) / K.fy * depth, -depth]


def _soup(T, K, seed, spread=1.0):
    """T dyadic triangles in front of the eye camera: vertices on a 1/16 grid around random centres over the image."""
    rng = np.random.default_rng(seed)
    half_w, half_h = K.W / 2.0 / K.fx * 2.0, K.H / 2.0 / K.fy * 2.0
    ctr = np.stack([rng.integers(-int(16 * half_w), int(16 * half_w) + 1, T) / 16.0,
                    rng.integers(-int(16 * half_h), int(16 * half_h) + 1, T) / 16.0,
                    -rng.integers(16, 64, T) / 16.0], axis=1)
    off = rng.integers(-int(8 * spread), int(8 * spread) + 1, (T, 3, 3)) / 16.0
    off[..., 2] = rng.integers(-4, 5, (T, 3)) / 16.0
    return (ctr[:, None, :] + off).astype(np.float32)


def _world(tri_cam, R, c):
    """Camera-frame dyadic triangles seen through (R, c): exact for a signed permutation R and a dyadic c."""
    return (np.asarray(tri_cam, np.float64) @ R.T + c).astype(np.float32)


def _dyadic_noise(shape, seed):
    return 1.0 + np.random.default_rng(seed).integers(-64, 65, shape) / 1024.0


def test_exact_family_bit_for_bit(lib, dev):
    K = _K(16, 16)
    sq = np.array([[[-0.9375, -0.9375, -1.0], [0.9375, -0.9375, -1.0], [0.9375, 0.9375, -1.0]],
                   [[-0.9375, -0.9375, -1.0], [0.9375, 0.9375, -1.0], [-0.9375, 0.9375, -1.0]]], np.float32)
    # scene 0 in the eye camera's frame, scene 1 the same geometry placed for the turned camera: B = 2, V = 2
    tri = np.stack([sq, _world(sq, TURNED_R, TURNED_C)])
    cams = np.stack([np.stack([EYE, TURNED]), np.stack([EYE, TURNED])])
    noise = _dyadic_noise((2, 2, K.H * K.W), 1)
    got = _call(lib, dev, tri, cams, K, noise=noise)
    want, _ = _ref(tri, cams, K, noise=noise)
    _assert_same(got, want, "square")
    _check_compaction(got, K)
    diag = np.arange(16) * 16 + np.arange(16)
    assert (got["triangle"][0, 0, diag] == 0).all() and (got["triangle"][1, 1, diag] == 0).all()   # the shared edge
    assert _bits_equal(got["range"][0, 0], got["range"][1, 1])
    # a soup with pixel centres on edges and vertices here and there
    K2 = _K(40, 24)
    soup = _soup(300, K2, 5, spread=3.0)
    tri2 = np.stack([soup, _world(soup, TURNED_R, TURNED_C)])
    got2 = _call(lib, dev, tri2, cams, K2)
    want2, _ = _ref(tri2, cams, K2)
    _assert_same(got2, want2, "soup")
    assert (got2["triangle"][0, 0] >= 0).mean() > 0.5 and _bits_equal(got2["triangle"][0, 0], got2["triangle"][1, 1])


@pytest.mark.parametrize("W,H", [(1, 1), (15, 16), (16, 16), (17, 16), (16, 17), (33, 47)])
def test_image_edges(lib, dev, W, H):
    K = _K(W, H)
    tri = _soup(90, K, 10 + W + H)[None]
    noise = _dyadic_noise((1, 2, W * H), W)
    cams = np.stack([EYE, RR.cam12(np.eye(3), np.array([0.25, -0.125, 0.5]))])[None]
    got = _call(lib, dev, tri, cams, K, noise=noise)
    want, _ = _ref(tri, cams, K, noise=noise)
    _assert_same(got, want, "%dx%d" % (W, H))
    _check_compaction(got, K)
    assert (got["triangle"] >= 0).any()


@pytest.mark.parametrize("T", sorted({0, 1, CHUNK - 1, CHUNK, CHUNK + 1, CAP - CHUNK, CAP - CHUNK + 1, CAP + 1,
                                      2 * CHUNK + 1}))
def test_triangle_count_edges(lib, dev, T):
    """The chunk size and the survivor list's flush threshold, both neighbours: every triangle covers the middle of
    the image, so the tiles there take every row of every chunk."""
    K = _K(33, 47)
    tri = _soup(T, K, 20 + T, spread=16.0)
    if T:
        tri[:, :, :2] *= 0.25                                          # crowd them over the centre tiles
    # scene 1: every triangle covers the whole image, nearer with a rising index: every tile's list takes all T rows
    z = -(2.0 - np.arange(T) / 512.0)
    layers = np.stack([np.stack([np.full(T, -16.0), np.full(T, -16.0), z], axis=1),
                       np.stack([np.full(T, 16.0), np.full(T, -16.0), z], axis=1),
                       np.stack([np.full(T, 0.0), np.full(T, 16.0), z], axis=1)], axis=1).astype(np.float32)
    both = np.stack([tri, layers])
    cams = np.stack([EYE[None]] * 2)
    got = _call(lib, dev, both, cams, K)
    want, _ = _ref(both, cams, K)
    _assert_same(got, want, "T = %d" % T)
    _check_compaction(got, K)
    if T:
        assert (got["triangle"][1] == T - 1).all()
    if T == 0:
        assert (got["triangle"] == -1).all() and np.isinf(got["range"]).all() and got["count"][0, 0] == 0
        assert np.isnan(got["points"]).all() and (got["pixel"] == -1).all()
    if T > CAP:
        centre = (K.H // 2) * K.W + K.W // 2
        assert got["triangle"][0, 0, centre] >= 0


def _geometry_cases():
    K = _K(32, 32)
    nan, inf = float("nan"), float("inf")
    cases = {}
    # vertices exactly on the tile boundary x = 16: one triangle on either side of it, one across
    cases["vertex_on_tile_boundary"] = [[_px(K, 16.0, 8.0, 2.0), _px(K, 22.0, 12.0, 2.0), _px(K, 16.0, 16.0, 2.0)],
                                        [_px(K, 16.0, 18.0, 2.0), _px(K, 16.0, 26.0, 2.0), _px(K, 10.0, 22.0, 2.0)],
                                        [_px(K, 16.0, 16.0, 1.0), _px(K, 16.0, 4.0, 1.0), _px(K, 4.0, 16.0, 1.0)]]
    # slivers that cover exactly one pixel centre, in each of the four tile corners that meet at (16, 16)
    sl = []
    for cxp, cyp in ((15.5, 15.5), (16.5, 15.5), (15.5, 16.5), (16.5, 16.5)):
        sl.append([_px(K, cxp - 0.25, cyp - 0.25, 1.0), _px(K, cxp + 0.25, cyp - 0.25, 1.0), _px(K, cxp, cyp + 0.25, 1.0)])
    cases["corner_slivers"] = sl
    # one vertex behind the camera plane, the visible part in front
    cases["straddles_camera_plane"] = [[[-1.0, -1.0, -1.0], [1.0, -1.0, -1.0], [0.0, 0.5, 1.0]],
                                       [[-0.5, 0.0, -2.0], [0.5, 0.0, -2.0], [0.0, 1.0, 0.0]]]
    cases["behind_the_camera"] = [[[-1.0, -1.0, 1.0], [1.0, -1.0, 1.0], [0.0, 1.0, 2.0]],
                                  [[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]],
                                  [_px(K, 2.0, 2.0, 3.0), _px(K, 12.0, 2.0, 3.0), _px(K, 2.0, 12.0, 3.0)]]
    cases["zero_area"] = [[[-1.0, -1.0, -2.0], [0.0, 0.0, -2.0], [1.0, 1.0, -2.0]],
                          [[0.5, 0.5, -1.0], [0.5, 0.5, -1.0], [0.5, 0.5, -1.0]],
                          [_px(K, 20.0, 20.0, 3.0), _px(K, 30.0, 20.0, 3.0), _px(K, 20.0, 30.0, 3.0)]]
    good = [[[-1.5, -1.5, -2.0], [1.5, -1.5, -2.0], [0.0, 1.5, -2.0]]]
    cases["nan_and_inf_rows"] = [[[nan, 0.0, -1.0], [1.0, 0.0, -1.0], [0.0, 1.0, -1.0]],
                                 [[-1.0, -1.0, -1.0], [inf, -1.0, -1.0], [0.0, 1.0, -1.0]],
                                 [[-1.0, -1.0, -inf], [1.0, -1.0, -1.0], [0.0, 1.0, -1.0]],
                                 [[nan, nan, nan], [nan, nan, nan], [nan, nan, nan]]] + good
    cases["coincident_duplicates"] = good * 3
    layer = lambda z: [[[-1.5, -1.5, z], [1.5, -1.5, z], [1.5, 1.5, z]], [[-1.5, -1.5, z], [1.5, 1.5, z], [-1.5, 1.5, z]]]  # noqa: E731
    cases["three_layers_reversed"] = layer(-3.0) + layer(-2.0) + layer(-1.0)
    return K, {k: np.asarray(v, np.float32) for k, v in cases.items()}


GEOMETRY_K, GEOMETRY = _geometry_cases()


@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_geometry_edges(lib, dev, name):
    K, tri = GEOMETRY_K, GEOMETRY[name]
    cams = np.stack([EYE, RR.cam12(np.eye(3), np.array([0.0, 0.0, 0.5]))])[None]
    got = _call(lib, dev, tri[None], cams, K)
    want, _ = _ref(tri[None], cams, K)
    _assert_same(got, want, name)
    _check_compaction(got, K)
    t0 = got["triangle"][0, 0]
    if name == "vertex_on_tile_boundary":
        cols = np.arange(K.H * K.W) % K.W
        assert set(cols[t0 == 0]) and cols[t0 == 0].min() == 16 and cols[t0 == 1].max() == 15
        assert cols[t0 == 2].max() == 15 and (t0 == 2).sum() > 20
    elif name == "corner_slivers":
        for i, (c, r) in enumerate(((15, 15), (16, 15), (15, 16), (16, 16))):
            assert np.array_equal(np.nonzero(t0 == i)[0], [r * K.W + c])
    elif name == "straddles_camera_plane":
        assert (t0 == 0).sum() > 20 and (t0 == 1).sum() > 5
    elif name == "behind_the_camera":
        assert set(np.unique(t0)) == {-1, 2}
    elif name == "zero_area":
        assert set(np.unique(t0)) == {-1, 2}
    elif name == "nan_and_inf_rows":
        alone = _call(lib, dev, tri[None, 4:], cams, K)                # the bad rows change no pixel
        assert _bits_equal(alone["range"], got["range"]) and _bits_equal(alone["points"], got["points"])
        assert np.array_equal(alone["triangle"], np.where(got["triangle"] >= 0, got["triangle"] - 4, -1))
        assert set(np.unique(t0)) == {-1, 4}
    elif name == "coincident_duplicates":
        assert set(np.unique(t0)) == {-1, 0}
    elif name == "three_layers_reversed":
        assert set(np.unique(t0)) <= {4, 5} | {-1, 2, 3, 0, 1} and (t0[(K.H // 2) * K.W + K.W // 2] in (4, 5))
        inner = t0.reshape(K.H, K.W)[8:24, 8:24]
        assert set(np.unique(inner)) == {4, 5}


def test_tri_count_and_nan_rows(lib, dev):
    K = _K(24, 20)
    soup = _soup(70, K, 3)
    tri = np.stack([soup, soup, soup])
    count = np.array([70, 23, 0], np.int32)
    tri[1, 23:] = np.nan
    tri[2, :] = np.nan
    got = _call(lib, dev, tri, np.stack([EYE[None]] * 3), K, count=count)
    want, _ = _ref(tri, np.stack([EYE[None]] * 3), K, count=count)
    _assert_same(got, want, "count")
    assert got["triangle"][1].max() < 23 and (got["triangle"][2] == -1).all() and got["count"][2, 0] == 0
    # counts outside [0, T] are clamped
    got2 = _call(lib, dev, tri[:2], np.stack([EYE[None]] * 2), K, count=np.array([1000, -5], np.int32))
    assert _bits_equal(got2["triangle"][0], got["triangle"][0]) and (got2["triangle"][1] == -1).all()


def test_max_depth_is_strict(lib, dev):
    K = _K(17, 17, max_depth=5.0, cx=8.5, cy=8.5)                      # pixel (8, 8) looks straight ahead: nor = 1
    plane = lambda z: np.array([[[-64, -64, z], [64, -64, z], [64, 64, z]], [[-64, -64, z], [64, 64, z], [-64, 64, z]]],  # noqa: E731
                               np.float32)
    tri = np.stack([plane(-5.0), plane(-4.75)])
    cams = np.stack([EYE[None]] * 2)
    got = _call(lib, dev, tri, cams, K)
    want, _ = _ref(tri, cams, K)
    _assert_same(got, want, "max_depth")
    centre = 8 * K.W + 8
    assert got["range"][0, 0, centre] == 5.0 and got["triangle"][0, 0, centre] >= 0
    assert centre not in got["pixel"][0, 0]                            # planar depth exactly max_depth: not kept
    assert got["count"][1, 0] == K.H * K.W and got["range"][1, 0].max() > 5.0   # the cut is on the planar depth


def test_compaction_and_noise(lib, dev):
    K = _K(40, 24)
    soup = _soup(120, K, 8)[None]
    cams = np.stack([EYE, TURNED])[None]
    P = K.H * K.W
    ones = _call(lib, dev, soup, cams, K, noise=np.ones((1, 2, P)))
    _check_compaction(ones, K)
    assert _bits_equal(ones["noisy"], ones["points"]) and 0 < ones["count"][0, 0] < P
    noise = 1.0 + 0.005 * np.random.default_rng(4).standard_normal((1, 2, P))
    got = _call(lib, dev, soup, cams, K, noise=noise)
    want, _ = _ref(soup, cams, K, noise=noise)
    _assert_same(got, want, "random multipliers")
    assert _bits_equal(got["points"], ones["points"]) and not _bits_equal(got["noisy"], got["points"])
    none = _call(lib, dev, soup, cams, K)
    assert _bits_equal(none["points"], ones["points"]) and _bits_equal(none["pixel"], ones["pixel"])


# ---- the fixture ------------------------------------------------------------------------------------------------------

def _fixture_call(golden):
    K = RR.intrinsics(float(golden["scale"]))
    views = RR.fixture_views(golden)
    cams = np.stack([RR.cam12(R, c) for _, R, c in views])[None]
    return K, views, cams, RR.fixture_scene(golden)[None]


def test_fixture_views(lib, dev, golden):
    K, views, cams, tri = _fixture_call(golden)
    P = K.H * K.W
    noise = 1.0 + 0.005 * np.random.default_rng(2).standard_normal((1, len(views), P))
    got = _call(lib, dev, tri, cams, K, noise=noise)
    _check_compaction(got, K)
    worst_range, worst_point = 0.0, 0.0
    for v, (name, R, c) in enumerate(views):
        decided = np.unpackbits(golden[name + "/decided"])[:P].astype(bool)
        want_t, want_r = golden[name + "/triangle"], golden[name + "/range"]
        assert np.array_equal(got["triangle"][0, v][decided], want_t[decided]), name
        hit = decided & (want_t >= 0)
        err = np.abs(got["range"][0, v][hit].astype(np.float64) - want_r[hit].astype(np.float64))
        rel = float((err / want_r[hit]).max())
        worst_range = max(worst_range, rel)
        assert rel <= 2.0 ** -22, (name, rel)
        assert np.isinf(got["range"][0, v][decided & (want_t < 0)]).all()
        # the clouds from the yardstick's range, at the pixels the kernel kept
        kept, pts, nsy = RR.unproject(want_r, want_t >= 0, np.arange(P), R, c, K, noise=noise[0, v])
        k = int(got["count"][0, v])
        pix = got["pixel"][0, v, :k]
        sel = decided[pix]
        assert np.array_equal(np.sort(pix[sel]), np.nonzero(kept & decided)[0]), name
        bound = 2.0 ** -22 * (want_r[pix].astype(np.float64) + np.abs(c).max())
        for cloud, ref in ((got["points"], pts), (got["noisy"], nsy)):
            e = np.abs(cloud[0, v, :, :k].T.astype(np.float64) - ref[pix].astype(np.float64)).max(axis=1)
            worst_point = max(worst_point, float((e[sel] / bound[sel]).max()))
            assert (e[sel] <= bound[sel]).all(), name
    print("fixture: worst range error %.3g of the range (bound %.3g); worst point error %.3g of its bound"
          % (worst_range, 2.0 ** -22, worst_point))


def test_python_interface_matches_the_entry(lib, dev, golden):
    from s4g_release_amd import postprocess as PP
    K, views, cams, tri = _fixture_call(golden)
    cfg = PP.RenderConfig(width=K.W, height=K.H, fx=K.fx, fy=K.fy, cx=K.cx, cy=K.cy,
                          camera_poses=tuple(tuple(golden["poses"][i]) for i in range(4)) + (tuple(golden["close_pose"]),))
    assert np.array_equal(cfg.cameras().numpy(), cams[0])
    P = K.H * K.W
    noise = 1.0 + 0.005 * np.random.default_rng(2).standard_normal((1, 5, P))
    raw = _call(lib, dev, tri, cams, K, noise=noise)
    labels = np.concatenate([np.full(len(golden["faces"]), 7, np.int32), np.full(12, 3, np.int32)])
    scene = PP.MeshScene(torch.from_numpy(tri[0]).to(dev), torch.from_numpy(labels).to(dev))
    out = PP.render_views(scene, config=cfg, noise=torch.from_numpy(noise).to(dev))
    for k, t in (("range", out.range), ("triangle", out.triangle), ("points", out.points), ("noisy", out.noisy),
                 ("pixel", out.pixel), ("count", out.count)):
        assert _bits_equal(t.cpu().numpy(), raw[k]), k
    lab = out.label.cpu().numpy()
    assert np.array_equal(lab, np.where(raw["triangle"] < 0, -1, np.where(raw["triangle"] < len(golden["faces"]), 7, 3)))
    clouds, count = out.clouds()
    assert clouds.shape == (5, 3, P) and count.shape == (5,) and count.dtype == torch.int32
    assert clouds.data_ptr() == out.noisy.data_ptr() and out.clouds(noisy=False)[0].data_ptr() == out.points.data_ptr()
    pts, nsy = out.dump(0, 4)
    k = int(raw["count"][0, 4])
    assert pts.shape == (k, 3) and np.array_equal(pts, raw["points"][0, 4, :, :k].T) and np.array_equal(
        nsy, raw["noisy"][0, 4, :, :k].T)
    # noise = False: no noisy cloud; noise = None: drawn on the device from the generator, reproducibly
    plain = PP.render_views(scene, config=cfg, noise=False)
    assert plain.noisy is None and torch.equal(plain.points.view(torch.int32), out.points.view(torch.int32))
    with pytest.raises(RuntimeError):
        plain.clouds()
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    a = PP.render_views(scene, config=cfg, generator=gen)
    gen.manual_seed(5)
    b = PP.render_views(scene, config=cfg, generator=gen)
    assert torch.equal(a.noisy.view(torch.int32), b.noisy.view(torch.int32))
    live = a.pixel[0, 0] >= 0
    ratio = (a.noisy[0, 0, :, live] - a.points[0, 0, :, live]).norm(dim=0) / a.range[0, 0][a.pixel[0, 0][live].long()]
    assert 0.003 < float(ratio.mean()) < 0.005                         # sigma 0.005: E|N(0, 1)| = 0.8
    # argument checks
    with pytest.raises(RuntimeError, match="CUDA"):
        PP.render_views(scene.triangles.cpu(), config=cfg)
    with pytest.raises(RuntimeError, match="float32"):
        PP.render_views(scene.triangles.double(), config=cfg)
    with pytest.raises(RuntimeError, match="int32"):
        PP.render_views(scene.triangles, tri_count=torch.zeros(1, dtype=torch.int64, device=dev), config=cfg)
    with pytest.raises(RuntimeError, match="noise"):
        PP.render_views(scene.triangles, config=cfg, noise=torch.ones((1, 5, P), device=dev))
    with pytest.raises(ValueError):
        PP.render_views(scene.triangles, config=PP.RenderConfig(width=4096, height=2048))
    with pytest.raises(ValueError, match="65535"):
        PP.render_views(scene.triangles[None, :4].expand(16384, 4, 3, 3), config=cfg, noise=False)


def test_full_size_call(lib, dev, golden):
    """640 x 480 x 4 on the fixture's scene.  The quarter-size fixture's pixel centres ((4 c + 2) / 700 against
    (col + 0.5) / 700) never coincide with full-size ones, so: a sample of pixels against the yardstick, and every
    pixel on the table box against the analytic slab intersection."""
    from s4g_release_amd import postprocess as PP
    tri = RR.fixture_scene(golden)
    out = PP.render_views(torch.from_numpy(tri).to(dev), noise=False)
    K = RR.intrinsics(1.0)
    P = K.H * K.W
    idx, rng, count = out.triangle.cpu().numpy()[0], out.range.cpu().numpy()[0], out.count.cpu().numpy()[0]
    n_mesh = len(golden["faces"])
    lo, hi = np.asarray(RR.TABLE_LO), np.asarray(RR.TABLE_HI)
    pix_all = np.arange(P)
    rays = np.stack([(pix_all % K.W + 0.5 - K.cx) / K.fx, (pix_all // K.W + 0.5 - K.cy) / K.fy, -np.ones(P)])
    nor = np.linalg.norm(rays, axis=0)
    for v, pose in enumerate(RR.CAMERA_POSE):
        R, c = RR.camera(pose)
        pix = np.sort(np.random.default_rng(40 + v).choice(P, 150, replace=False))
        res = RR.render_ref(tri, R, c, K, pixels=pix)
        d = res.decided
        assert d.mean() > 0.98
        assert np.array_equal(idx[v][pix][d], res.triangle[d]), v
        hit = d & (res.triangle >= 0)
        assert (np.abs(rng[v][pix][hit].astype(np.float64) - res.range[hit]) <= 2.0 ** -22 * res.range[hit]).all()
        assert int(count[v]) == int((idx[v] >= 0).sum())               # everything here is nearer than 5 m
        assert (idx[v] >= n_mesh).sum() > 50000 and ((idx[v] >= 0) & (idx[v] < n_mesh)).sum() > 2000
        # the table: where the ray enters the box clear of its silhouette and the kernel saw the box, the face and
        # the range are the slab's
        dw = (R @ rays).T
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - c) / dw, (hi - c) / dw
        near, far = np.minimum(t0, t1), np.maximum(t0, t1)
        tn, tf = near.max(axis=1), far.min(axis=1)
        axis = near.argmax(axis=1)
        face = 2 * axis + (dw[pix_all, axis] < 0)
        on_box = idx[v] >= n_mesh
        clear = (tf - tn > 1e-4) & (np.sort(near, axis=1)[:, 2] - np.sort(near, axis=1)[:, 1] > 1e-4)
        sel = on_box & clear
        assert sel.sum() > 40000
        assert np.array_equal((idx[v][sel] - n_mesh) // 2, face[sel]), v
        assert np.allclose(rng[v][sel], (tn * nor)[sel], rtol=2e-6)
        assert not (clear & (tn < tf) & (tf > 0) & (idx[v] < 0)).any()  # no ray through the box misses


# ---- invariance -------------------------------------------------------------------------------------------------------

def _random_scene(T, seed):
    rng = np.random.default_rng(seed)
    ctr = np.stack([rng.uniform(-0.35, 0.35, T), rng.uniform(-0.3, 0.3, T), rng.uniform(0.75, 1.0, T)], axis=1)
    return (ctr[:, None, :] + rng.uniform(-0.08, 0.08, (T, 3, 3))).astype(np.float32)


def test_batch_invariance(lib, dev):
    K = RR.intrinsics(0.1)
    cams4 = np.stack([RR.cam12(*RR.camera(p)) for p in RR.CAMERA_POSE])
    a, b, c = _random_scene(700, 1), _random_scene(300, 2), _random_scene(513, 3)
    T = 700
    tri = np.full((3, T, 3, 3), np.nan, np.float32)
    tri[0], tri[1, :300], tri[2, :513] = a, b, c
    noise = 1.0 + 0.005 * np.random.default_rng(9).standard_normal((3, 4, K.H * K.W))
    batch = _call(lib, dev, tri, np.stack([cams4] * 3), K, count=np.array([700, 300, 513], np.int32), noise=noise)
    alone = _call(lib, dev, b[None], cams4[None], K, noise=noise[1:2])
    for k in ("range", "triangle", "points", "noisy", "pixel", "count"):
        assert _bits_equal(batch[k][1:2], alone[k]), k
    assert (alone["triangle"] >= 0).mean() > 0.2


def test_run_to_run_graph_and_chain(dev, golden):
    """Twice the same bits; no host read in render_views -> process_views -> trace; a captured graph replays them."""
    from s4g_release_amd import postprocess as PP
    from s4g_release_amd import preprocess
    K = RR.intrinsics(0.25)
    cfg = PP.RenderConfig(width=K.W, height=K.H, fx=K.fx, fy=K.fy, cx=K.cx, cy=K.cy)
    tri = torch.from_numpy(np.stack([RR.fixture_scene(golden)[-3000:], _random_scene(3000, 6)])).to(dev)
    noise = torch.from_numpy(1.0 + 0.005 * np.random.default_rng(1).standard_normal((2, 4, K.H * K.W))).to(dev)

    def run():
        views = PP.render_views(tri, config=cfg, noise=noise)
        clouds, count = views.clouds()
        pv = preprocess.process_views(clouds, count)
        return views, pv, pv.trace(views.clouds(noisy=False)[0])

    def bits(o):
        views, pv, ref = o
        return [t.view(torch.int32) for t in (views.range, views.triangle, views.points, views.noisy, views.pixel,
                                              views.count, pv.points, pv.index_in_ref, pv.count, ref)]

    eager, again = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(bits(eager), bits(again)))
    views, pv, ref = eager
    assert int(pv.count.min()) > 50                                    # the chain carries points to its end
    # it keeps only rendered rows: every traced index is below the view's count, and the traced reference row is the
    # noise-free point of the same pixel
    idx, cnt = pv.index_in_ref.cpu().numpy(), views.count.reshape(-1).cpu().numpy()
    for r in range(idx.shape[0]):
        k = int(pv.count[r])
        assert (idx[r, :k] >= 0).all() and (idx[r, :k] < cnt[r]).all() and (idx[r, k:] == -1).all()
        want = views.points.reshape(-1, 3, K.H * K.W)[r][:, torch.from_numpy(idx[r, :k]).long().to(dev)]
        assert torch.equal(ref[r, :, :k], want) and bool(ref[r, :, k:].isnan().all())
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
    with torch.cuda.graph(graph):                                      # a host read would fail the capture
        out = run()
    for t in bits(out):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert all(torch.equal(x, y) for x, y in zip(bits(eager), bits(out)))


# ---- refusals ---------------------------------------------------------------------------------------------------------

REFUSALS = [("views", dict(B=65536, V=1)), ("views_product", dict(B=256, V=256)), ("negative_batch", dict(B=-1)),
            ("pixels", dict(H=2049, W=2048)), ("wide", dict(H=1, W=(1 << 22) + 1)), ("triangles", dict(T=1 << 24)),
            ("negative_triangles", dict(T=-1)), ("fx_zero", dict(fx=0.0)), ("fy_negative", dict(fy=-700.0)),
            ("fx_nan", dict(fx=float("nan"))), ("fy_inf", dict(fy=float("inf"))), ("cx_nan", dict(cx=float("nan"))),
            ("height_zero", dict(H=0)), ("width_negative", dict(W=-4))]


@pytest.mark.parametrize("name,told", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_outputs_untouched(lib, dev, name, told):
    K = _K(16, 16)
    tri = _soup(5, K, 1)[None]
    assert _call(lib, dev, tri, EYE[None, None], K, noise=np.ones((1, 1, 256)), expect=EINVAL, told=told), name


def test_workspace_refusals(lib, dev):
    K = _K(16, 16)
    tri = _soup(5, K, 1)[None]
    assert _call(lib, dev, tri, EYE[None, None], K, expect=EWORKSPACE, ws_short=1)
    assert _call(lib, dev, tri, EYE[None, None], K, expect=EWORKSPACE, null_ws=True)
    assert lib.s4g_render_views_workspace_bytes(65536, 1, 5, 16, 16) == 0
    assert lib.s4g_render_views_workspace_bytes(1, 1, 1 << 24, 16, 16) == 0
    assert lib.s4g_render_views_workspace_bytes(1, 1, 5, 2049, 2048) == 0
    assert lib.s4g_render_views_workspace_bytes(1, 4, (1 << 24) - 1, 2048, 2048) > 0
    # the limits themselves are served: B * V = 65 535 views of one pixel
    Kp = _K(1, 1)
    one = np.array([[[-1, -1, -1], [1, -1, -1], [0, 1, -1]]], np.float32)
    tri = one[None].copy()
    cams = np.broadcast_to(EYE, (1, 65535, 12)).copy()
    got = _call(lib, dev, tri, cams, Kp)
    assert (got["triangle"] == 0).all() and (got["count"] == 1).all() and (got["range"] == got["range"][0, 0, 0]).all()
