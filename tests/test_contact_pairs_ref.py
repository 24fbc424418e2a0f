"""The float64 yardstick of the contact model's per-object data (tests/contact_pairs_ref.py) against the fixture the
reference's own `cache_contact_pair`, `_estimate_grasp_quality` and `get_frame_neighbor` produced
(tests/golden/contact_pairs.npz, tools/gen_golden_contact_pairs.py), on the CPU.

The yardstick must reproduce the reference on every decided row (the rule is in the yardstick's docstring; eps0 is the
fixture's own measurement of the reference's fp32 error), the fixture must meet its conditions, and every planted
mistake must change at least 20 kept rows: a yardstick that agreed with the reference by accident, or a fixture whose
kept rows did not exercise a rule, would show here.  The grading mistakes run on the first 300 graded pairs and the
pair mistakes on the first 1 500 points of the cloud (a random subset: the sampler's order), to keep this quick."""
import os
import re

import numpy as np
import pytest

from tests import contact_pairs_ref as CP
from tests import golden_util as GU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB_PAIRS, SUB_POINTS, MIN_CHANGED = 300, 1500, 20


@pytest.fixture(scope="module")
def fx():
    g = GU.load("contact_pairs.npz")
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def cloud(fx):
    return fx["points"].astype(np.float64), fx["normals"].astype(np.float64)


@pytest.fixture(scope="module")
def graded(fx, cloud):
    """The yardstick's grade of the fixture's subset, and the reference's verdicts as dense arrays."""
    row, col = fx["pair_row"][fx["subset"]], fx["pair_col"][fx["subset"]]
    g = CP.grade(cloud[0], row, col, float(fx["eps0"][0]))
    ref_valid = np.zeros_like(g["valid"])
    ref_valid[fx["frame_pair"], fx["frame_roll"]] = True
    ref_score = np.zeros_like(g["score"])
    ref_score[fx["frame_pair"], fx["frame_roll"]] = fx["search_score"]
    return g, ref_valid, ref_score, row, col


def test_fixture_conditions(fx, graded):
    g, ref_valid, _, _, _ = graded
    assert os.path.getsize(os.path.join(GU.GOLDEN, "contact_pairs.npz")) < 1000000
    assert len(fx["subset"]) >= 1000 and len(fx["global_to_local"]) >= 2000
    assert 0 < float(fx["eps0"][0]) <= 1e-6
    # eps0 is twice the largest scaled distance of the reference's own fp32 coordinates from float64
    T, xlen = CP.pair_frames(fx["points"].astype(np.float64), *graded[3:])
    assert np.isclose(2 * float((fx["local_error"].astype(np.float64) * xlen).max()), float(fx["eps0"][0]), rtol=1e-6)
    d = g["decided"]
    assert d.mean() >= 0.5 and (d & ref_valid).sum() >= 1000, (d.mean(), (d & ref_valid).sum())


def test_yardstick_reproduces_the_pair_list(fx, cloud):
    pr = CP.pairs(*cloud)
    undecided = int((~pr["decided"]).sum()) + pr["near"].shape[1]
    assert undecided <= 0.01 * len(fx["pair_row"])
    ours = set(zip(pr["row"][pr["decided"]].tolist(), pr["col"][pr["decided"]].tolist()))
    theirs = set(zip(fx["pair_row"].tolist(), fx["pair_col"].tolist()))
    maybe = set(zip(pr["row"][~pr["decided"]].tolist(), pr["col"][~pr["decided"]].tolist())) | \
        set(zip(*pr["near"].tolist()))
    assert ours <= theirs and theirs - ours <= maybe
    if not maybe:
        assert np.array_equal(pr["row"], fx["pair_row"]) and np.array_equal(pr["col"], fx["pair_col"])   # and the order
        assert np.abs(pr["score"] - fx["pair_score"]).max() < 1e-12
    # the strided subset is what the generator says it is
    assert np.array_equal(fx["subset"], np.arange(0, len(fx["pair_row"]), int(fx["params"][2])))


def test_yardstick_reproduces_the_grading(fx, cloud, graded):
    g, ref_valid, ref_score, row, col = graded
    d = g["decided"]
    assert np.array_equal(g["valid"][d], ref_valid[d])
    assert np.array_equal(g["score"][d], ref_score[d])                      # exact fp32 functions of integers
    # the append order: ascending pair * T + roll
    key = fx["frame_pair"].astype(np.int64) * len(CP.THETA_SEARCH) + fx["frame_roll"]
    assert (np.diff(key) > 0).all()
    fr = CP.frames(g)
    at = {(p, t): i for i, (p, t) in enumerate(zip(fr["pair"].tolist(), fr["roll"].tolist()))}
    idx, sure = CP.nearest(cloud[0], fr["global_to_local"])
    compared = 0
    for f, (p, t) in enumerate(zip(fx["frame_pair"].tolist(), fx["frame_roll"].tolist())):
        if not d[p, t]:
            continue
        i = at[(p, t)]
        # the reference's frame: fp32 axes normalised in fp32 and torch.inverse; both lose 1 / |x| in the x and z axes
        assert np.abs(fr["global_to_local"][i] - fx["global_to_local"][f]).max() < 2e-6 / g["xlen"][p], (p, t)
        assert fx["antipodal_score"][f] == fx["pair_score"][fx["subset"][p]]
        if sure[i]:
            compared += 1
            assert idx[i] == fx["frame_point_index"][f], (p, t)
    assert compared >= 1000


def _changed_grading(fx, cloud, graded, sabotage):
    g, ref_valid, ref_score, row, col = graded
    s = CP.grade(cloud[0], row[:SUB_PAIRS], col[:SUB_PAIRS], float(fx["eps0"][0]), sabotage)
    d = g["decided"][:SUB_PAIRS]
    return int(((s["valid"] != ref_valid[:SUB_PAIRS]) | (s["score"] != ref_score[:SUB_PAIRS]))[d].sum())


@pytest.mark.parametrize("sabotage", ["threshold_le", "dw_order", "max_dw", "no_third", "no_min", "rolls_reversed",
                                      "no_move_back", "back_without_close"])
def test_a_grading_mistake_shows(fx, cloud, graded, sabotage):
    assert _changed_grading(fx, cloud, graded, sabotage) >= MIN_CHANGED


def test_no_grading_mistake_changes_nothing(fx, cloud, graded):
    assert _changed_grading(fx, cloud, graded, None) == 0


@pytest.mark.parametrize("sabotage", ["no_triu", "one_sided_cos"])
def test_a_pair_mistake_shows(fx, cloud, sabotage):
    P, Nn = cloud[0][:SUB_POINTS], cloud[1][:SUB_POINTS]
    inside = (fx["pair_row"] < SUB_POINTS) & (fx["pair_col"] < SUB_POINTS)
    theirs = dict(zip(zip(fx["pair_row"][inside].tolist(), fx["pair_col"][inside].tolist()),
                      fx["pair_score"][inside].tolist()))

    def changed(sab):
        pr = CP.pairs(P, Nn, sab)
        ours = dict(zip(zip(pr["row"].tolist(), pr["col"].tolist()), pr["score"].tolist()))
        return len(set(ours) ^ set(theirs)) + sum(1 for k in set(ours) & set(theirs) if abs(ours[k] - theirs[k]) > 1e-12)

    assert changed(None) == 0
    assert changed(sabotage) >= MIN_CHANGED


def test_no_clip_needs_a_close_pair():
    """`no_clip` shows only where two points are nearer than 0.1 mm, which a cloud thinned to one point per 4 mm voxel
    does not hold twenty times: the clip is pinned on a hand-built cloud instead (the eleven other mistakes are
    counted on the fixture)."""
    P = np.array([[0, 0, 0], [0.00005, 0, 0]], np.float64)
    Nn = np.array([[1, 0, 0], [-1, 0, 0]], np.float64)
    assert len(CP.pairs(P, Nn)["row"]) == 0                                  # score 0.25 under the clip
    assert len(CP.pairs(P, Nn, "no_clip")["row"]) == 1


def test_a_nearest_point_mistake_shows(fx, cloud, graded):
    g, _, _, row, col = graded
    fr = CP.frames(g)
    keep = g["decided"][fr["pair"], fr["roll"]]
    idx, sure = CP.nearest(cloud[0], fr["global_to_local"][:600])
    mid = (cloud[0][row[fr["pair"][:600]]] + cloud[0][col[fr["pair"][:600]]]) / 2
    bad, _ = CP.nearest(cloud[0], fr["global_to_local"][:600], "nearest_from_midpoint", mid)
    assert int(((idx != bad) & sure & keep[:600]).sum()) >= MIN_CHANGED


def _declared(text, name):
    return re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S)) is not None


def test_header_and_cabi_name_the_entries():
    from s4g_release_amd import _cabi
    header = open(os.path.join(ROOT, "include", "s4g_ops.h")).read()
    abi = header[header.index(" * 14:"):header.index("#define S4G_ABI_VERSION")]
    for name in ("s4g_contact_pairs_f32", "s4g_contact_pairs_workspace_bytes", "s4g_contact_pair_grade_f32",
                 "s4g_contact_pair_grade_workspace_bytes"):
        assert name in abi and _declared(header, name) and name in _cabi.SIGNATURES, name
    assert _cabi.S4G_ABI_VERSION == 14 and "#define S4G_ABI_VERSION 14" in header
    src = open(os.path.join(ROOT, "s4g_release_amd", "csrc", "contact_pairs.hip")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n, word in enumerate(("formed in double", "not finite", "rounded once", "configuration"), 1):
        assert "(%d)" % n in src and word in src and word in header and word in doc, word


def test_config_matches_the_reference_constants():
    from s4g_release_amd import postprocess as PP
    cfg = PP.ContactPairConfig()
    assert cfg.half_bottom_space == CP.HALF_BOTTOM_SPACE and cfg.max_distance == CP.HALF_BOTTOM_SPACE * 2
    assert tuple(cfg.theta_search) == CP.THETA_SEARCH and tuple(cfg.width_shift) == CP.WIDTH_SHIFT
    assert (cfg.min_points, cfg.back_threshold, cfg.finger_threshold, cfg.cos_threshold, cfg.gasket_radius) == \
        (50, 0, 0, 0.95, 0.012)
    # the roll table: the reference's fp32 inverse, within fp32 of the exact one
    L = cfg.local_to_local_search().numpy().astype(np.float64)
    assert L.shape == (12, 4, 4) and np.abs(L - CP.local_to_local_search()).max() < 1e-6
    t = cfg.tables().numpy()
    assert t.shape == (12 * 12 + 6,) and t.dtype == np.float32
    assert np.array_equal(t[144:], np.float32([-0.012 - 0.015, -0.012 + 0.015, -0.012, 0.012 - 0.015, 0.012 + 0.015, 0.012]))
    for bad in (dict(theta_search=tuple(range(17))), dict(width_shift=(0,) * 5), dict(theta_search=())):
        with pytest.raises(ValueError):
            PP.ContactPairConfig(**bad).check()
    # quat2mat written out: a quarter turn about z
    R = PP.quaternion_matrix((np.sqrt(0.5), 0, 0, np.sqrt(0.5))).numpy()
    assert np.abs(R - np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]])).max() < 1e-15
