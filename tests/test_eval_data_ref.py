"""CPU tests of the evaluation data's test infrastructure: the fixture the reference's own `finger_hand_view` and
`finger_hand_scene` produced (tests/golden/eval_data.npz, tools/gen_golden_eval_data.py) against the float64 yardstick
(tests/eval_data_ref.py), the yardstick's sensitivity to the mistakes it must see, and the C boundary."""
import os
import re

import numpy as np
import pytest

from tests import eval_data_ref as ED


@pytest.fixture(scope="module")
def fixture_case():
    fx = ED.load_fixture()
    case = ED.case_of(fx)
    return fx, case, ED.label64(*case)


def test_fixture_agrees_with_the_yardstick(fixture_case):
    fx, case, (v, t) = fixture_case
    kf, kg = ED.keep_masks(v, t)
    assert np.array_equal(kf, fx["keep_frames"]) and np.array_equal(kg, fx["keep_grasps"])
    valid = fx["ref_valid"]
    F = len(valid)
    assert kf.sum() >= 0.75 * F and kg.sum() >= 0.75 * valid.sum()
    assert np.array_equal((v["index"] >= 0)[kf], valid[kf])
    assert np.array_equal(v["index"], fx["index"]) and np.array_equal(t["stage"], fx["stage"])
    row = np.full(F, -1)
    row[valid] = np.arange(valid.sum())
    g = np.nonzero(kf & valid)[0]
    assert np.abs(fx["ref_baseline_frame"][row[g]] - v["g2l"][g]).max() <= 1e-5
    g = np.nonzero(kg)[0]
    assert np.array_equal(fx["ref_non_collision"][row[g]], t["non_collision"][g])
    assert np.array_equal(fx["ref_single_label"][row[g]], t["single_label"][g])
    a, b = fx["ref_score"][row[g]].astype(np.float64), t["score"][g]
    assert ((np.abs(a - b) <= 1e-5) | (np.isnan(a) & np.isnan(b))).all()
    assert float(fx["margin"][1]) <= 1e-5
    # the sets: on kept rows no member is ambiguous and the yardstick's set is the stored one
    off = fx["set_offset"]
    for j, f in enumerate(fx["set_rows"]):
        assert np.array_equal(v["regions"][f]["certain"], fx["set_index"][off[j]:off[j + 1]].astype(np.int64)), f
    have = ED.counts(v, t, kf, kg)
    for name, n in ED.REQUIRED.items():
        assert have[name] >= n, (name, have[name])


def test_stored_maps_are_the_projection_of_the_stored_sets(fixture_case):
    from s4g_release_amd.postprocess import ProjectionConfig
    from tests import close_region_ref as CRR
    fx, case, _ = fixture_case
    cfg, proj = case[6], ProjectionConfig()
    off = fx["stored_offset"]
    for j in range(len(fx["stored_rows"])):
        p, n = fx["stored_points"][:, off[j]:off[j + 1]], fx["stored_normals"][:, off[j]:off[j + 1]]
        m64, _ = CRR.projection64(p, n, proj, cfg.search)
        assert np.abs(fx["maps"][j] - m64).max() <= max(float(fx["margin"][0]), 1e-6)


@pytest.mark.parametrize("name", ED.SABOTAGES)
def test_every_sabotage_alters_kept_rows(fixture_case, name):
    fx, case, base = fixture_case
    keep = (fx["keep_frames"], fx["keep_grasps"])
    assert len(ED.SABOTAGES) >= 10
    assert ED.altered_rows(case, name, base, keep) >= 20


def test_constants_of_the_fixture_are_the_config(fixture_case):
    fx, case, _ = fixture_case
    s = case[6].search
    want = [s.finger_length, s.bottom_length, s.half_bottom_space, s.half_hand_thickness, s.half_bottom_width,
            s.table_height, s.table_collision_offset, s.num_points_threshold, s.back_collision_threshold,
            s.finger_collision_threshold, s.close_region_min_points, s.neighbor_depth]
    assert np.allclose(fx["constants"][:12], want, rtol=0, atol=1e-7)
    assert abs(fx["constants"][12] - 0.02 - case[6].region()) <= 1e-12        # SAMPLE_REGION - 0.02 (:59)


def test_header_and_cabi_carry_the_symbols():
    from s4g_release_amd import _cabi
    header = open(os.path.join(ED.ROOT, "include", "s4g_ops.h")).read()
    assert re.search(r"#define S4G_ABI_VERSION 14\b", header) and _cabi.S4G_ABI_VERSION == 14
    for name in ("s4g_eval_view_search_f32", "s4g_eval_view_search_workspace_bytes", "s4g_eval_scene_grade_f32",
                 "s4g_eval_scene_grade_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _cabi.SIGNATURES, name
    c = ED.constants_in_source()
    assert c["EVD_GX"] * c["EVD_SLOTS"] > 0 and c["EVS_GX"] * c["EVS_SLOTS"] > 0


def test_public_names():
    import s4g_release_amd as pkg
    from s4g_release_amd import postprocess as PP
    for name in ("label_eval_view", "grade_eval_view_frames", "grade_eval_scene_frames"):
        assert callable(getattr(pkg, name)) and callable(getattr(PP, name))
    cfg = PP.EvalDataConfig()
    assert cfg.grasp_num == 2000 and cfg.min_neighbours == 5 and abs(cfg.region() - (0.75 + 0.015 - 0.02)) < 1e-12
