"""The crop, voxel and radius-outlier kernels at their edges (tests/preprocess_edges.py lists the scenes and why;
tests/test_preprocess_edges.py keeps that list honest on the CPU).  Every comparison is bit for bit: masks and indices
against `counts_ref(...) > nb` / oracle/preprocess.py, voxel means against `voxel_ref`.  The C entries are also called
directly on sentinel-filled buffers: return codes, N = 0, and nothing written past an output.  Every refusal case is
one the entry rejects before it launches anything, and is handed valid buffers all the same."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import preprocess as OP
from tests import preprocess_edges as PE

pytestmark = pytest.mark.gpu

RADIUS_CASES = PE.radius_cases()
BY_ID = {i: (get, nb) for i, get, nb in RADIUS_CASES}


@pytest.fixture(scope="module")
def PP():
    from s4g_release_amd import functions, preprocess
    functions.set_distance_mode("strict")
    return preprocess


@pytest.fixture(scope="module")
def lib():
    from s4g_release_amd import _cabi
    return _cabi.lib()


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)      # a copy: the scenes are read-only and shared


def _mask(PP, scene, nb, dev):
    return PP.radius_outlier_mask(_dev(scene.points, dev), nb, scene.radius).cpu().numpy()


def _explain(got, want, scene):
    bad = np.nonzero(got != want)[0]
    return "%s: %d of %d points differ, first %s" % (scene.name, len(bad), scene.n, bad[:8].tolist())


# ===================================================================================================== radius outliers
@pytest.mark.parametrize("case", [i for i, _, _ in RADIUS_CASES])
def test_radius_outlier_mask_equals_the_reference(PP, dev, case):
    get, nb = BY_ID[case]
    scene = get()
    want = scene.counts() > nb
    got = _mask(PP, scene, nb, dev)
    assert got.dtype == np.bool_ and got.shape == want.shape
    assert np.array_equal(got, want), _explain(got, want, scene)


@pytest.mark.parametrize("case", PE.FMAD_CASES)
def test_radius_outlier_mask_under_the_fmad_contract(PP, dev, case):
    from s4g_release_amd import functions
    get, nb = BY_ID[case]
    scene = get()
    want = scene.counts(True) > nb
    functions.set_distance_mode("fmad")
    try:
        got = _mask(PP, scene, nb, dev)
    finally:
        functions.set_distance_mode("strict")
    assert np.array_equal(got, want), _explain(got, want, scene)
    if case.startswith("pairs"):                  # the scene separates the two contracts
        assert not np.array_equal(want, scene.counts() > nb)
        assert np.array_equal(_mask(PP, scene, nb, dev), scene.counts() > nb)


def test_radius_outlier_mask_is_the_same_twice(PP, dev):
    get, nb = BY_ID[PE.TWICE_CASE]
    scene = get()
    a, b = _mask(PP, scene, nb, dev), _mask(PP, scene, nb, dev)
    assert a.tobytes() == b.tobytes()
    assert np.array_equal(a, scene.counts() > nb)


# ============================================================================================================== voxel
def _voxel_check(PP, dev, pts, v):
    got = PP.voxel_down_sample(_dev(pts, dev), v).cpu().numpy()
    origin, dims = OP.voxel_grid(pts, v)
    want = PE.voxel_ref(pts, v, origin, dims)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), "first differing cell %d" % np.nonzero((got != want).any(axis=0))[0][0]
    return want


@pytest.mark.parametrize("fill", PE.VOXEL_FILLS)
@pytest.mark.parametrize("n", PE.VOXEL_N)
def test_voxel_down_sample_fills(PP, dev, n, fill):
    pts, v = PE.voxel_fill_scene(n, fill)
    want = _voxel_check(PP, dev, pts, v)
    assert want.shape[1] == {"own-cell": n, "one-cell": 1}.get(fill, want.shape[1])


@pytest.mark.parametrize("k", range(len(PE.BITS_LADDER)))
def test_voxel_down_sample_key_widths(PP, dev, k):
    pts, v, dims = PE.voxel_bits_scene(k)
    _voxel_check(PP, dev, pts, v)


def test_voxel_down_sample_points_on_cell_bounds(PP, dev):
    _voxel_check(PP, dev, *PE.voxel_bounds_scene())


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_voxel_down_sample_refuses_non_finite_coordinates(PP, dev, axis, bad):
    pts = PE.tabletop(500).copy()
    pts[axis, 123] = bad
    with pytest.raises(RuntimeError, match="non-finite coordinates"):
        PP.voxel_down_sample(_dev(pts, dev), 0.005)


def test_pre_processing_with_a_nan_point_needs_the_crop(PP, dev):
    cloud = PE.tabletop(15000, scene=11).copy()
    cloud[2] += np.float32(2.145)                 # into the camera frame: the table top just above the box's floor
    cloud[:, 5] = np.nan                          # what a depth camera emits for a missing return
    cloud[1, 4000] = np.inf
    with pytest.raises(RuntimeError, match="non-finite coordinates"):
        PP.pre_processing(_dev(cloud, dev), num_input=2048, seed=3)
    pts, proc = PP.pre_processing(_dev(cloud, dev), num_input=2048, seed=3, workspace=PP.WORKSPACE)
    cropped = cloud[:, OP.filter_work_space(cloud, PP.WORKSPACE)]
    assert 0 < cropped.shape[1] < cloud.shape[1] - 2 and np.isfinite(cropped).all()
    want = OP.pre_processing(cropped, PP.VOXEL_SIZE, PP.NUM_POINTS_THRESHOLD, PP.RADIUS_THRESHOLD, 2048, 3)
    assert pts.shape == (3, 2048) and np.array_equal(pts.cpu().numpy(), want)


# =============================================================================================================== crop
@pytest.mark.parametrize("n", PE.CROP_N)
def test_crop_keep_patterns(PP, dev, n):
    for pattern in PE.CROP_PATTERNS:
        pts, keep = PE.crop_scene(n, pattern)
        got = PP.filter_work_space(_dev(pts, dev), PE.CROP_BOX).cpu().numpy()
        assert got.dtype == np.int64
        assert np.array_equal(got, OP.filter_work_space(pts, PE.CROP_BOX)), pattern
        assert np.array_equal(got, np.nonzero(keep)[0]), pattern


def test_crop_drops_non_finite_points(PP, dev):
    pts = PE.crop_nonfinite_scene()
    got = PP.filter_work_space(_dev(pts, dev), PE.CROP_BOX).cpu().numpy()
    assert np.array_equal(got, OP.filter_work_space(pts, PE.CROP_BOX)) and len(got) == pts.shape[1] - 27


def test_crop_is_strict_on_all_six_faces(PP, dev):
    pts, inside = PE.crop_faces_scene()
    got = PP.filter_work_space(_dev(pts, dev), PE.CROP_BOX).cpu().numpy()
    assert np.array_equal(got, OP.filter_work_space(pts, PE.CROP_BOX)) and np.array_equal(got, np.nonzero(inside)[0])


@pytest.mark.parametrize("box", PE.CROP_EMPTY_BOXES)
def test_crop_with_an_empty_box_keeps_nothing(PP, dev, box):
    pts, _ = PE.crop_scene(1025, "all")
    got = PP.filter_work_space(_dev(pts, dev), box)
    assert got.numel() == 0 and len(OP.filter_work_space(pts, box)) == 0


# ========================================================================================================= C contracts
def _box6(box):
    return (ctypes.c_float * 6)(*[float(v) for v in box])


def _stream():
    from s4g_release_amd import functions
    return functions._stream()


def test_crop_entry_contract(lib, dev):
    from s4g_release_amd import _cabi
    n = 2049
    pts, keep = PE.crop_scene(n, "random")
    x = _dev(pts, dev)
    index = torch.full((n + 64,), -7, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        assert lib.s4g_crop_indices_f32(x.data_ptr(), n, _box6(PE.CROP_BOX), index.data_ptr(), count.data_ptr(),
                                        _stream()) == 0
        c = int(count.item())
        assert c == keep.sum() and np.array_equal(index[:c].cpu().numpy(), np.nonzero(keep)[0])
        assert (index[c:] == -7).all()                                     # nothing past the kept indices
        # N = 0: null cloud and index, the count is written
        count.fill_(5)
        assert lib.s4g_crop_indices_f32(None, 0, _box6(PE.CROP_BOX), None, count.data_ptr(), _stream()) == 0
        assert int(count.item()) == 0
        # refusals (valid buffers everywhere but the argument under test)
        count.fill_(-7)
        index.fill_(-7)
        assert lib.s4g_crop_indices_f32(x.data_ptr(), n, None, index.data_ptr(), count.data_ptr(),
                                        _stream()) == _cabi.S4G_EINVAL
        assert lib.s4g_crop_indices_f32(x.data_ptr(), n, _box6(PE.CROP_BOX), index.data_ptr(), None,
                                        _stream()) == _cabi.S4G_EINVAL
        assert lib.s4g_crop_indices_f32(x.data_ptr(), -1, _box6(PE.CROP_BOX), index.data_ptr(), count.data_ptr(),
                                        _stream()) == _cabi.S4G_EINVAL
        torch.cuda.synchronize()
        assert int(count.item()) == -7 and (index == -7).all()


def _voxel_call(lib, dev, pts, voxel, origin, dims, ws_short=0, null_ws=False, n=None):
    """s4g_voxel_down_sample_f32 on sentinel-filled buffers of the full size -> (rc, out, count)."""
    n_real = pts.shape[1]
    n = n_real if n is None else n
    x = _dev(pts, dev)
    out = torch.full((3, max(n_real, 1)), -12345.0, dtype=torch.float32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int32, device=dev)
    nbytes = lib.s4g_voxel_down_sample_workspace_bytes(n_real)
    ws = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=dev)
    o3 = (ctypes.c_float * 3)(*[float(v) for v in origin])
    d3 = (ctypes.c_int32 * 3)(*[int(v) for v in dims])
    with torch.cuda.device(dev):
        rc = lib.s4g_voxel_down_sample_f32(x.data_ptr(), n, float(voxel), o3, d3, out.data_ptr(), count.data_ptr(),
                                           None if null_ws else ws.data_ptr(), 0 if null_ws else nbytes - ws_short,
                                           _stream())
        torch.cuda.synchronize()
    return rc, out.cpu().numpy(), int(count.item())


def test_voxel_entry_contract(lib, dev):
    from s4g_release_amd import _cabi
    pts, v = PE.voxel_fill_scene(2049, "mix")
    origin, dims = OP.voxel_grid(pts, v)
    want = PE.voxel_ref(pts, v, origin, dims)
    rc, out, count = _voxel_call(lib, dev, pts, v, origin, dims)
    assert rc == 0 and count == want.shape[1] < pts.shape[1]
    assert out[:, :count].tobytes() == want.tobytes()
    assert (out[:, count:] == -12345.0).all()                              # the columns past the cells are untouched
    rc, out, count = _voxel_call(lib, dev, pts, v, origin, dims, n=0)
    assert rc == 0 and count == 0 and (out == -12345.0).all()
    assert lib.s4g_voxel_down_sample_workspace_bytes(0) == 0 and lib.s4g_voxel_down_sample_workspace_bytes(-3) == 0
    refused = [
        (0.0, origin, dims), (-0.005, origin, dims), (float("nan"), origin, dims),
        (v, origin, (0, 1, 1)), (v, origin, (4, -1, 4)), (v, origin, (4, 4, 0)),
        (v, origin, (65536, 65536, 1)), (v, origin, (2048, 2048, 1024)),
        (v, (float("nan"), 0.0, 0.0), dims), (v, (0.0, float("inf"), 0.0), dims), (v, (0.0, 0.0, float("-inf")), dims),
    ]
    for voxel, o, d in refused:
        rc, out, count = _voxel_call(lib, dev, pts, voxel, o, d)
        assert rc == _cabi.S4G_EINVAL, (voxel, o, d)
        assert count == -7 and (out == -12345.0).all(), (voxel, o, d)
    for kwargs in ({"ws_short": 256}, {"ws_short": 1}, {"null_ws": True}):
        rc, out, count = _voxel_call(lib, dev, pts, v, origin, dims, **kwargs)
        assert rc == _cabi.S4G_EWORKSPACE, kwargs
        assert count == -7 and (out == -12345.0).all(), kwargs


def test_voxel_entry_clamps_points_outside_the_grid(lib, dev):
    pts, v, origin, dims = PE.voxel_clamp_scene()
    want = PE.voxel_ref(pts, v, origin, dims)
    rc, out, count = _voxel_call(lib, dev, pts, v, origin, dims)
    assert rc == 0 and count == want.shape[1]
    assert out[:, :count].tobytes() == want.tobytes() and (out[:, count:] == -12345.0).all()


def _radius_call(lib, dev, pts, radius, nb, ws_short=0, null_ws=False, flags=0):
    """s4g_radius_outlier_mask_f32 with keep sized N + 64 and filled with 7 -> (rc, keep)."""
    n = pts.shape[1]
    x = _dev(pts, dev)
    keep = torch.full((n + 64,), 7, dtype=torch.uint8, device=dev)
    nbytes = lib.s4g_radius_outlier_workspace_bytes(n)
    ws = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.s4g_radius_outlier_mask_f32(x.data_ptr(), n, float(radius), int(nb), keep.data_ptr(),
                                             None if null_ws else ws.data_ptr(), 0 if null_ws else nbytes - ws_short,
                                             flags, _stream())
        torch.cuda.synchronize()
    return rc, keep.cpu().numpy()


def test_radius_entry_contract(lib, dev):
    from s4g_release_amd import _cabi
    assert lib.s4g_radius_outlier_workspace_bytes(0) == 0 and lib.s4g_radius_outlier_workspace_bytes(-1) == 0
    assert lib.s4g_radius_outlier_workspace_bytes(PE.GR_MAX_POINTS + 1) == 0
    assert lib.s4g_radius_outlier_workspace_bytes(PE.GR_MAX_POINTS) > 0
    scene, nb = PE.ladder_scene(8193), PE.LADDER_NB
    rc, keep = _radius_call(lib, dev, scene.points, scene.radius, nb)
    assert rc == 0 and np.array_equal(keep[:scene.n], (scene.counts() > nb).astype(np.uint8))
    assert (keep[scene.n:] == 7).all()                                     # nothing past keep[N - 1]
    for kwargs in ({"ws_short": 256}, {"null_ws": True}):
        rc, keep = _radius_call(lib, dev, scene.points, scene.radius, nb, **kwargs)
        assert rc == _cabi.S4G_EWORKSPACE and (keep == 7).all(), kwargs
    for radius, bad_nb in ((0.0, nb), (-0.02, nb), (float("nan"), nb), (scene.radius, -1)):
        rc, keep = _radius_call(lib, dev, scene.points, radius, bad_nb)
        assert rc == _cabi.S4G_EINVAL and (keep == 7).all(), (radius, bad_nb)


def test_radius_entry_scans_large_clouds_without_a_workspace(lib, dev):
    scene, nb = PE.ladder_scene(PE.GR_MAX_POINTS + 1), PE.LADDER_NB
    rc, keep = _radius_call(lib, dev, scene.points, scene.radius, nb, null_ws=True)
    assert rc == 0 and np.array_equal(keep[:scene.n], (scene.counts() > nb).astype(np.uint8))
    assert (keep[scene.n:] == 7).all()
