"""CPU tests of the drop-in boundary: the C-ABI library loads (no GPU needed)
and exports every symbol include/s4g_ops.h declares; the Python operator API
keeps the reference's names; and the product path has no CPU fallback."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "s4g_ops.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(s4g_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_boundary():
    syms = _declared_symbols()
    for required in ("s4g_fps_f32", "s4g_ball_query_f32", "s4g_group_points_f32",
                     "s4g_group_points_backward_f32", "s4g_gather_points_f32", "s4g_three_nn_f32",
                     "s4g_three_interpolate_f32", "s4g_three_interpolate_backward_f32"):
        assert required in syms


def test_library_exports_every_declared_symbol():
    from s4g_release_amd import _cabi
    assert os.path.exists(_cabi.LIB_PATH), "build libs4g_hip.so first (__graft_entry__.build())"
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in _declared_symbols():
        assert hasattr(L, name), "libs4g_hip.so does not export %s" % name
    # and the ctypes table covers the header one to one
    assert sorted(_cabi.SIGNATURES) == _declared_symbols()
    assert _cabi.lib().s4g_abi_version() == _cabi.S4G_ABI_VERSION
    assert _cabi.lib().s4g_error_string(-1)


def test_operator_api_names_match_reference():
    from s4g_release_amd import functions as F, pn2_ext
    for name in ("gather_points", "farthest_point_sample", "ball_query", "group_points",
                 "search_nn_distance", "feature_interpolate", "gather_knn", "query_and_group",
                 "furthest_point_sample", "three_nn", "three_interpolate"):
        assert callable(getattr(F, name))
    for name in ("ball_query", "group_points_forward", "group_points_backward",
                 "farthest_point_sample", "point_search", "interpolate_forward",
                 "interpolate_backward"):
        assert callable(getattr(pn2_ext, name))


def test_no_cpu_fallback():
    from s4g_release_amd import functions as F
    pts = torch.zeros(1, 3, 8)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        F.farthest_point_sample(pts, 4)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        F.ball_query(pts, pts, 0.1, 4)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        F.search_nn_distance(pts, pts, 3)


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "s4g_release_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f


def test_ab_knobs_are_ignored_without_the_master_switch(monkeypatch):
    """include/s4g_ops.h: the A/B / test knobs are read only with S4G_TEST_KNOBS=1 (tests/conftest.py sets it).  Host side
    (`_cabi.knob`) and library side (`s4g_test_knobs_enabled`, csrc/s4g_common.h s4g::knob) agree; the production surface
    is the seven variables the header lists and nothing else in the package reads the environment."""
    import re
    from s4g_release_amd import _cabi
    monkeypatch.setenv("S4G_GEMM_FUSE2", "0")
    assert _cabi.knob("S4G_GEMM_FUSE2", "1") == "0"
    monkeypatch.delenv("S4G_TEST_KNOBS")
    assert _cabi.knob("S4G_GEMM_FUSE2", "1") == "1" and _cabi.knob("S4G_GEMM_FUSE2") is None
    monkeypatch.setenv("S4G_TEST_KNOBS", "yes")                    # only the literal "1" enables
    assert _cabi.knob("S4G_GEMM_FUSE2", "1") == "1"
    L = ctypes.CDLL(_cabi.LIB_PATH)                                 # no compute call: the symbol and its answer
    L.s4g_test_knobs_enabled.restype = ctypes.c_int
    assert L.s4g_build_variants() == 0                              # kept in the ABI; no library carries variants
    assert L.s4g_test_knobs_enabled() == 0
    monkeypatch.setenv("S4G_TEST_KNOBS", "1")
    assert L.s4g_test_knobs_enabled() == 1
    # every direct environment read in the package is one of the production variables (or torch.distributed's own)
    allowed = {"S4G_TEST_KNOBS", "S4G_HIP_LIB", "S4G_GEMM_MODE", "S4G_DIST_MODE", "S4G_BACKWARD", "S4G_GEO_STREAMS",
               "S4G_DENSE_STREAMS", "NCCL_MAX_NCHANNELS", "WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR"}
    pkg = os.path.join(ROOT, "s4g_release_amd")
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            for name in re.findall(r'os\.environ(?:\.get|\.setdefault)?[\(\[]\s*"([A-Z0-9_]+)"', src):
                assert name in allowed, (f, name)
    csrc = os.path.join(pkg, "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            src = open(os.path.join(csrc, f)).read()
            direct = re.findall(r'(?<![:\w])getenv\("([A-Z0-9_]+)"\)', src)
            assert set(direct) <= {"S4G_TEST_KNOBS"}, (f, direct)


def test_knob_table_lists_exactly_the_knobs_that_are_read_and_tested():
    """The A/B list of include/s4g_ops.h is the set of knobs the code reads (`_cabi.knob("NAME"` in the package,
    `s4g::knob("NAME")` in csrc/), and every one of them is set by at least one test: a knob nothing drives is dead
    code and goes, together with the path it selects."""
    header = open(os.path.join(ROOT, "include", "s4g_ops.h")).read()
    table = header[header.index("A/B AND TEST KNOBS"):]
    table = table[:table.index("*/")]
    listed = set(re.findall(r"\bS4G_[A-Z0-9_]+", table)) - {"S4G_TEST_KNOBS"}
    assert listed, "the knob table of include/s4g_ops.h was not found"
    pkg = os.path.join(ROOT, "s4g_release_amd")
    read = set()
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py"):
            read |= set(re.findall(r'_cabi\.knob\(\s*"(S4G_[A-Z0-9_]+)"', open(os.path.join(pkg, f)).read()))
    csrc = os.path.join(pkg, "csrc")
    for dirpath, _, files in os.walk(csrc):
        for f in sorted(files):
            if f.endswith((".hip", ".h", ".inc")):
                read |= set(re.findall(r'(?<![\w.])(?:s4g::)?knob\(\s*"(S4G_[A-Z0-9_]+)"\s*\)',
                                       open(os.path.join(dirpath, f)).read()))
    assert read == listed, (sorted(read - listed), sorted(listed - read))
    tests_dir = os.path.join(ROOT, "tests")
    driven = set()
    for dirpath, _, files in os.walk(tests_dir):
        for f in sorted(files):
            if f.endswith(".py"):
                driven |= set(re.findall(r'setenv\(\s*"(S4G_[A-Z0-9_]+)"', open(os.path.join(dirpath, f)).read()))
    assert listed <= driven, sorted(listed - driven)
