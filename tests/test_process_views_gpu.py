"""GPU tests of `process_views` (csrc/process_views.hip) against the numpy yardstick (tests/process_views_ref.py) and,
per scene, against the shipped single-cloud kernels it must reproduce: `s4g_crop_indices_f32` ->
`s4g_voxel_down_sample_f32` over the same grid -> `s4g_radius_outlier_mask_f32`.  Every comparison is bit for bit.

The C entry is called with the views inside a NaN-filled buffer, and every output and the workspace inside a poisoned
buffer with guard bytes on both sides, checked after the call."""
import ctypes

import numpy as np
import pytest
import torch

from tests import preprocess_edges as PE
from tests import process_views_ref as PV

pytestmark = pytest.mark.gpu

GUARD = 256                # bytes on both sides of every output and of the workspace
POISON = 0xA5
PAD = 64                   # NaN floats on both sides of the views


@pytest.fixture(scope="module")
def PP():
    from s4g_release_amd import functions, preprocess
    functions.set_distance_mode("strict")
    return preprocess


@pytest.fixture(scope="module")
def lib():
    from s4g_release_amd import _cabi
    return _cabi.lib()


def _stream():
    from s4g_release_amd import functions
    return functions._stream()


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)


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

    def untouched(self, names):
        torch.cuda.synchronize(self.dev)
        return all(bool((self.bufs[k][0] == POISON).all()) for k in names)


def _grid_args(cfg, origin=None, dims=None):
    o, d = PV.voxel_grid(cfg)
    o = o if origin is None else origin
    d = d if dims is None else dims
    return ((ctypes.c_float * 6)(*[float(v) for v in cfg.workspace]), float(np.float32(cfg.voxel_size)),
            (ctypes.c_float * 3)(*[float(v) for v in o]), (ctypes.c_int32 * 3)(*[int(v) for v in d]))


def _call(lib, dev, clouds, count, cfg, flags=0, expect=0, ws_short=0, null_ws=False, shape=None, dims=None):
    """s4g_process_views_f32 through the C ABI -> PV.Result of numpy arrays (expect == 0), or whether every output and the
    workspace are untouched (a refusal).  shape: the (B, N) the entry is told, where it is not the buffers'."""
    B, _, N = clouds.shape
    xbuf = torch.full((B * 3 * N + 2 * PAD,), float("nan"), dtype=torch.float32, device=dev)
    xbuf[PAD:PAD + B * 3 * N] = _t(clouds, dev).reshape(-1)
    x = xbuf[PAD:PAD + B * 3 * N]
    cnt = None if count is None else _t(np.asarray(count, np.int32), dev)
    g = _Guarded(dev)
    p_points = g.add("points", (B, 3, N), torch.float32)
    p_index = g.add("index", (B, N), torch.int32)
    p_counts = g.add("counts", (B, 3), torch.int32)
    tB, tN = (B, N) if shape is None else shape
    nbytes = int(lib.s4g_process_views_workspace_bytes(B, N))
    p_ws = g.add("workspace", (max(nbytes, 1),), torch.uint8)
    box, voxel, o3, d3 = _grid_args(cfg, dims=dims)
    with torch.cuda.device(dev):
        rc = lib.s4g_process_views_f32(x.data_ptr(), None if cnt is None else cnt.data_ptr(), tB, tN, box, voxel, o3, d3,
                                       float(cfg.radius), int(cfg.nb_points), p_points, p_index, p_counts,
                                       None if null_ws else p_ws, 0 if null_ws else nbytes - ws_short, flags, _stream())
    assert rc == expect, rc
    if expect != 0:
        return g.untouched(("points", "index", "counts", "workspace"))
    out = g.read()
    c = out["counts"]
    return PV.Result(out["points"], out["index"], c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy())


def _shipped(PP, lib, dev, cloud, live, cfg):
    """One view through the shipped single-cloud kernels -> (points (3, K), crop, voxel, K)."""
    x = _t(cloud[:, :live], dev)
    kept = PP.filter_work_space(x, cfg.workspace)
    q = x[:, kept].contiguous()
    n = q.size(1)
    if n == 0:
        return np.zeros((3, 0), np.float32), 0, 0, 0
    out = torch.empty((3, n), dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = lib.s4g_voxel_down_sample_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _, voxel, o3, d3 = _grid_args(cfg)
    with torch.cuda.device(dev):
        assert lib.s4g_voxel_down_sample_f32(q.data_ptr(), n, voxel, o3, d3, out.data_ptr(), count.data_ptr(),
                                             ws.data_ptr(), nbytes, _stream()) == 0
    v = int(count.item())
    means = out[:, :v].contiguous()
    keep = PP.radius_outlier_mask(means, cfg.nb_points, cfg.radius)
    pts = means[:, keep].cpu().numpy()
    return pts, n, v, pts.shape[1]


def _explain(got, want):
    for name, a, b in zip(PV.Result._fields, got, want):
        if np.asarray(a).tobytes() != np.asarray(b).tobytes():
            bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
            return "%s differs at %s" % (name, bad[:4].tolist())
    return "equal"


def _check_case(PP, lib, dev, case, flags=0, fmad=False):
    got = _call(lib, dev, case.clouds, case.count, case.cfg, flags)
    want = PV.process_views_ref(case.clouds, case.count, case.cfg, fmad)
    assert PV.same(got, want), "%s: %s" % (case.name, _explain(got, want))
    B, _, N = case.clouds.shape
    for b in range(B):
        pts, crop, vox, k = _shipped(PP, lib, dev, case.clouds[b], N if case.count is None else int(case.count[b]),
                                     case.cfg)
        assert (crop, vox, k) == (got.crop_count[b], got.voxel_count[b], got.count[b]), (case.name, b)
        assert got.points[b, :, :k].tobytes() == pts.tobytes(), (case.name, b)
        assert np.isnan(got.points[b, :, k:]).all() and (got.index_in_ref[b, k:] == -1).all(), (case.name, b)
    return got


# ============================================================================== the yardstick and the shipped kernels
@pytest.mark.parametrize("n", PV.SIZES)
def test_sizes(PP, lib, dev, n):
    got = _check_case(PP, lib, dev, PV.size_case(n))
    assert got.crop_count[2] == 0 and got.count[2] == 0
    if n >= 63:
        assert 0 < got.count[0] < got.voxel_count[0] < got.crop_count[0] < n


@pytest.mark.parametrize("name", [c.name for c in PV.constructions()])
def test_constructions(PP, lib, dev, name):
    _check_case(PP, lib, dev, {c.name: c for c in PV.constructions()}[name])


def test_chunk_crossing(PP, lib, dev):
    case = PV.chunk_case()
    assert PV.key_plan(case.cfg, *case.clouds.shape[::2]) == (28, 16) and case.clouds.shape[0] == 17
    got = _check_case(PP, lib, dev, case)
    assert (got.count > 0).all() and (got.count < got.voxel_count).all()


@pytest.mark.parametrize("name", ["distance-r", "n257"])
def test_fmad_contract(PP, lib, dev, name):
    from s4g_release_amd import _cabi, functions
    case = PV.size_case(257) if name == "n257" else {c.name: c for c in PV.constructions()}[name]
    functions.set_distance_mode("fmad")
    try:
        _check_case(PP, lib, dev, case, flags=_cabi.S4G_FLAG_FMAD, fmad=True)
    finally:
        functions.set_distance_mode("strict")


def test_data_gen_constants_on_a_table_top_cloud(PP, lib, dev):
    """The generator's constants (201 x 201 x 161 cells, 23 cell bits) on a table-top cloud in the camera frame."""
    cloud = PE.tabletop(6000, scene=11).copy()
    cloud[2] += np.float32(2.145)
    cloud[:, 5] = np.nan
    case = PV.Case("data-gen", np.stack([cloud, PE.tabletop(6000, scene=12) + np.float32([[0], [0], [2.145]])]),
                   np.array([6000, 4097], np.int32), PV.DATA_GEN)
    got = _check_case(PP, lib, dev, case)
    assert (0 < got.count).all() and (got.count <= got.voxel_count).all() and (got.voxel_count <= got.crop_count).all()
    assert (got.crop_count > 1000).all()


# ================================================================================= the wrapper: invariance, graphs
def _fields(r):
    return [r.points, r.index_in_ref, r.crop_count, r.voxel_count, r.count]


def _equal(a, b):
    return all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(a, b))


def test_batch_invariance_determinism_and_graph(PP, dev):
    from s4g_release_amd.preprocess import ViewProcessingConfig
    cfg = ViewProcessingConfig(*PV.LATTICE)
    n = 1025
    a, b, c = PV.surface_view(n, 21), PV.surface_view(n, 22), PV.surface_view(n, 23)
    three = _t(np.stack([a, b, c]), dev)
    counts = _t(np.array([700, n, 333], np.int32), dev)
    batch = PP.process_views(three, counts, cfg)
    want = PV.process_views_ref(np.stack([a, b, c]), [700, n, 333], PV.LATTICE)
    got = PV.Result(*[t.cpu().numpy() for t in _fields(batch)])
    assert PV.same(got, want), _explain(got, want)
    assert batch.crop_count.is_contiguous() and batch.count.dtype == torch.int32
    again = PP.process_views(three, counts, cfg)
    assert _equal(_fields(batch), _fields(again))
    for k, live in enumerate((700, n, 333)):
        alone = PP.process_views(three[k], counts[k:k + 1], cfg)             # (3, N): gets a leading 1
        assert alone.unbatched and alone.points.shape == (1, 3, n)
        assert _equal([t[0] for t in _fields(alone)], [t[k] for t in _fields(batch)]), k
    # without a count every row is live
    full = PP.process_views(three[1:2], None, cfg)
    assert _equal([t[0] for t in _fields(full)], [t[1] for t in _fields(batch)])
    # one capture on one stream, replayed
    run = lambda: PP.process_views(three, counts, cfg)                       # noqa: E731
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for t in _fields(out):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert _equal(_fields(batch), _fields(out))


def test_trace_gathers_the_reference(PP, dev):
    from s4g_release_amd.preprocess import ViewProcessingConfig
    cfg = ViewProcessingConfig(*PV.LATTICE)
    n = 300
    views = np.stack([PV.surface_view(n, 31), PV.surface_view(n, 32)])
    ref = np.random.default_rng(5).random((2, 3, n)).astype(np.float32)
    out = PP.process_views(_t(views, dev), _t(np.array([n, 100], np.int32), dev), cfg)
    traced = out.trace(_t(ref, dev)).cpu().numpy()
    idx, k = out.index_in_ref.cpu().numpy(), out.count.cpu().numpy()
    for b in range(2):
        assert 0 < k[b] < n
        assert traced[b, :, :k[b]].tobytes() == ref[b][:, idx[b, :k[b]]].tobytes()
        assert np.isnan(traced[b, :, k[b]:]).all()


# ======================================================================================================== bad calls
def test_refusals_come_before_any_launch(PP, lib, dev):
    from s4g_release_amd import _cabi
    case = PV.size_case(257)
    args = (lib, dev, case.clouds, case.count, case.cfg)
    # the grid does not contain the crop box: bounds inside it on one axis, at the lower and at the upper face
    inside_lo = case.cfg._replace(voxel_bounds=((0.0, 0.125, 0.0), (1.0, 1.0, 1.0)))
    inside_hi = case.cfg._replace(voxel_bounds=((0.0, 0.0, 0.0), (1.0, 1.0, 0.875)))
    for cfg in (inside_lo, inside_hi):
        assert _call(lib, dev, case.clouds, case.count, cfg, expect=_cabi.S4G_EINVAL), cfg.voxel_bounds
        with pytest.raises(ValueError, match="do not contain the workspace"):
            PP.process_views(_t(case.clouds, dev), None, PP.ViewProcessingConfig(*cfg))
    assert _call(*args, expect=_cabi.S4G_EINVAL, dims=(129, 120, 129))       # the upper y face lies in cell 120
    assert _call(*args, expect=_cabi.S4G_EINVAL, dims=(129, 129, 0))
    assert _call(*args, expect=_cabi.S4G_EINVAL, dims=(65536, 65536, 1))
    # B * N >= 2^31 and B > 65 535 (the buffers stay small: nothing may be read or written)
    assert _call(*args, expect=_cabi.S4G_EINVAL, shape=(65535, 32769))
    assert _call(*args, expect=_cabi.S4G_EINVAL, shape=(65536, 1))
    assert _call(*args, expect=_cabi.S4G_EINVAL, shape=(-1, 257))
    assert lib.s4g_process_views_workspace_bytes(65535, 32769) == 0 and lib.s4g_process_views_workspace_bytes(0, 5) == 0
    for bad in (case.cfg._replace(radius=0.0), case.cfg._replace(radius=float("nan")), case.cfg._replace(radius=1e19),
                case.cfg._replace(nb_points=-1)):
        assert _call(lib, dev, case.clouds, case.count, bad, expect=_cabi.S4G_EINVAL), bad
    for kwargs in ({"ws_short": 256}, {"ws_short": 1}, {"null_ws": True}):
        assert _call(*args, expect=_cabi.S4G_EWORKSPACE, **kwargs), kwargs
    with pytest.raises(RuntimeError, match="int32"):
        PP.process_views(_t(case.clouds, dev), _t(np.array([1, 2, 3], np.int64), dev), PP.ViewProcessingConfig(*case.cfg))
    with pytest.raises(RuntimeError, match=r"\(B, 3, N\)"):
        PP.process_views(_t(case.clouds[:, :2], dev), None, PP.ViewProcessingConfig(*case.cfg))


def test_empty_shapes(PP, lib, dev):
    case = PV.size_case(63)
    got = _call(lib, dev, case.clouds[:, :, :0], None, case.cfg)
    assert (got.crop_count == 0).all() and (got.voxel_count == 0).all() and (got.count == 0).all()
    out = PP.process_views(_t(case.clouds[:, :, :0], dev), None, PP.ViewProcessingConfig(*case.cfg))
    assert out.points.shape == (3, 3, 0) and int(out.count.abs().sum()) == 0


# ============================================================================================================ chain
def test_chain_into_match_scene_frames(PP, dev):
    """process_views -> .trace(reference) -> match_scene_frames: the padded arrays give the live rows the trimmed arrays
    give, and no candidate in the padding."""
    from s4g_release_amd import postprocess as PO
    rng = np.random.default_rng(77)
    cfg = PO.PrecomputedViewConfig()
    L, T = cfg.search.shape
    M, n = 2500, 900
    scene_pts = np.stack([rng.uniform(-0.15, 0.15, M), rng.uniform(-0.15, 0.15, M), rng.uniform(0.752, 0.85, M)])
    nrm = rng.normal(size=(3, M))
    nrm /= np.linalg.norm(nrm, axis=0)
    h = np.where(np.abs(nrm[2:3]) < 0.9, [[0.0], [0.0], [1.0]], [[1.0], [0.0], [0.0]])
    p = np.cross(nrm.T, h.T)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    frames = np.stack([-nrm.T, -p, np.cross(-nrm.T, -p)], 2).astype(np.float32)
    scene = PO.DarbouxScene(*[_t(a, dev) for a in (
        scene_pts.astype(np.float32), nrm.astype(np.float32), rng.integers(0, 4, M).astype(np.int32), frames, frames,
        rng.integers(0, 120, (M, L, T)).astype(np.int32), rng.integers(0, 120, (M, L, T)).astype(np.int32),
        rng.uniform(0, 1, (M, L, T)).astype(np.float32), rng.uniform(0, 1, (M, L, T)).astype(np.float32))])
    pick = rng.choice(M, n)
    ref = (scene_pts[:, pick] + rng.normal(0, 0.0005, (3, n))).astype(np.float32)
    noisy = (ref + rng.normal(0, 0.001, (3, n))).astype(np.float32)
    noisy[:, ::50] = np.nan                                                   # missing returns
    camera = _t(np.array([0.5, -0.3, 1.55], np.float32), dev)
    out = PP.process_views(_t(noisy, dev))                                    # the generator's constants
    k = int(out.count[0])
    assert 50 < k < int(out.voxel_count[0]) <= int(out.crop_count[0]) < n
    traced = out.trace(_t(ref, dev))
    padded = PO.match_scene_frames(traced, out.points, scene, camera, cfg)
    trimmed = PO.match_scene_frames(traced[:, :, :k].contiguous(), out.points[:, :, :k].contiguous(), scene, camera, cfg)
    fc = int(trimmed.frame_count[0])
    assert int((trimmed.nearest >= 0).sum()) > 40 and fc > 5
    assert int(padded.frame_count[0]) == fc
    assert torch.equal(padded.frame_index[0, :fc], trimmed.frame_index[0, :fc]) and (padded.frame_index[0, fc:] == -1).all()
    assert (padded.candidate_i32[0, k:] == 0).all() and (padded.nearest[0, k:] == -1).all()
    for name in ("nearest", "normals", "flipped_i32", "frames", "pre_search", "pre_antipodal", "mask", "candidate_i32"):
        a, b = getattr(padded, name), getattr(trimmed, name)
        a = a[:, :, :k] if name == "normals" else a[:, :k]
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), name
