"""The float64 yardstick of the Darboux frame estimation (tests/darboux_ref.py) against the fixture the reference's own
`_estimate_frame` produced (tests/golden/darboux.npz), the C ABI's declarations, the index selection of
torch_single_view_point_cloud.py:53 and the mapping of `valid_index` to cloud indices.  No GPU."""
import os

import numpy as np
import torch

from tests import darboux_ref as DR
from tests import golden_util as GU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_yardstick_reproduces_the_fixture():
    fx = GU.load("darboux.npz")
    y = DR.frames64(fx["cloud"], fx["normals"], fx["index"], float(fx["radius"][0]))
    assert np.array_equal(y["count"], fx["count"])
    few = fx["count"] < 5
    assert few.sum() >= 5 and (fx["frames"][few] == np.eye(3)).all() and (y["frames"][few] == np.eye(3)).all()
    assert np.array_equal(DR.decided(y), ~few)                         # the fixture keeps k < 5 and the decided frames
    assert DR.flip_distance(fx["frames"], y["frames"]).max() <= 1e-12
    on = fx["labels"][fx["index"]]
    assert ((on == 1) & ~few).sum() >= 300 and ((on == 2) & ~few).sum() >= 300
    assert 0 < float(fx["margin"][0]) < 1e-6 and float(fx["radius"][0]) == 0.01
    # the reference's frames are rotations: orthonormal, determinant +1
    R = fx["frames"][~few]
    assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() < 1e-6 and np.abs(np.linalg.det(R) - 1).max() < 1e-6


def test_the_flip_is_a_half_turn_about_the_approach_axis():
    fx = GU.load("darboux.npz")
    R = fx["frames"][fx["count"] >= 5][:20]
    half_turn = np.diag(DR.FLIP)
    assert np.array_equal(R * DR.FLIP, R @ half_turn)
    assert (DR.flip_distance(R @ half_turn, R) == 0).all() and not DR.sign_agrees(R @ half_turn, R).any()


def test_the_cabi_declares_both_entries_and_the_header_names_them():
    from s4g_release_amd import _cabi
    header = open(os.path.join(ROOT, "include", "s4g_ops.h")).read()
    for name, nargs in (("s4g_darboux_frames_f32", 16), ("s4g_darboux_frames_workspace_bytes", 3)):
        assert name in _cabi.SIGNATURES and len(_cabi.SIGNATURES[name][1]) == nargs
        assert name + "(" in header
        decl = header[header.rindex(name + "("):]                      # (the declaration follows its comment)
        assert decl[:decl.index(");")].count(",") == nargs - 1
    assert _cabi.S4G_ABI_VERSION == 14 and "#define S4G_ABI_VERSION 14" in header
    import s4g_release_amd
    assert callable(s4g_release_amd.estimate_frames) and callable(s4g_release_amd.label_view)


def test_the_index_selection_is_line_53():
    from s4g_release_amd import postprocess as PP
    fx = GU.load("darboux.npz")
    sr = float(fx["sample_region"][0])
    assert sr == PP.LocalSearchConfig().table_height + PP.SAMPLE_REGION_OFFSET
    cloud = fx["cloud"]
    other = cloud[:, ::-1].copy()
    other[2, :40] = np.float32(sr)                                     # ON the threshold: not selected (strict)
    index, count = PP.sample_frame_index(torch.from_numpy(np.stack([cloud, other])), sr)
    assert index.dtype == torch.int32 and count.dtype == torch.int64 and tuple(index.shape) == (2, cloud.shape[1])
    for b, c in enumerate((cloud, other)):
        want = DR.sample_indices(c, sr)
        assert int(count[b]) == len(want) and 0 < len(want) < c.shape[1]
        assert np.array_equal(index[b, :len(want)].numpy(), want) and (index[b, len(want):] == -1).all()
    assert int(count[0]) == int(fx["sample_count"][0])
    assert np.isin(fx["index"], index[0].numpy()).all()
    none, zero = PP.sample_frame_index(torch.zeros(1, 3, 5), sr)       # nothing above the region
    assert int(zero[0]) == 0 and (none == -1).all()


def test_cloud_index_maps_frame_rows_to_cloud_indices():
    from s4g_release_amd import postprocess as PP
    frame_index = torch.tensor([[7, 3, 9, -1], [0, 5, -1, -1]], dtype=torch.int32)
    valid_index = torch.tensor([[0, 2, -1, -1], [1, -1, -1, -1]], dtype=torch.int32)
    got = PP.map_cloud_index(valid_index, frame_index)
    assert got.dtype == torch.int32 and got.tolist() == [[7, 9, -1, -1], [5, -1, -1, -1]]


def test_the_yardsticks_own_edge_cases():
    """A self-test of the yardstick alone (it says nothing about the kernel; tests/test_darboux_gpu.py holds the
    kernel to these same cases): k < 5 leaves the identity, padding rows are zero, a normal field whose smallest
    eigenvector is the normal itself is degenerate."""
    cloud = np.zeros((3, 6), np.float32)
    cloud[0, 5] = 1.0                                                  # five points together, one far away
    normals = np.tile(np.array([[0], [0], [1]], np.float32), (1, 6))
    y = DR.frames64(cloud, normals, np.array([0, 5, -1]), 0.01)
    assert list(y["count"]) == [5, 1, 0]
    assert (y["frames"][1] == np.eye(3)).all() and not y["frames"][2].any() and not y["estimated"][1:].any()
    cloud, normals = DR.parallel_patch()
    y = DR.frames64(cloud, normals, np.array([0]), 0.01)
    assert y["count"][0] == cloud.shape[1] and y["degenerate"][0] and not y["frames"][0].any()
