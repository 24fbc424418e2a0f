"""CPU tests of the fast pipeline's view stage: the fixture the reference's own `_find_match` and `finger_hand` produced
(tests/golden/precomputed_view.npz, tools/gen_golden_precomputed_view.py) against the float64 yardstick
(tests/precomputed_view_ref.py), what the fixture must hold, the mistakes it must see, and the refusals of the public
entry points, which need no GPU."""
import os

import numpy as np
import pytest
import torch

from tests import precomputed_view_ref as PV

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "precomputed_view.npz")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def base(fx):
    cfg = PV.default_config()
    return PV.label64(fx["reference_cloud"], fx["cloud"], PV.scene_of(fx), fx["camera"], cfg, float(fx["radius"][0]))


def test_fixture_equals_the_yardstick_on_kept_rows(fx, base):
    m, g = base
    kp, kf = fx["keep_points"].astype(bool), fx["keep_frames"].astype(bool)
    ykp, ykf = PV.decided(m, g)
    assert np.array_equal(kp, ykp) and np.array_equal(kf, ykf)
    fi = fx["ref_frame_index"].astype(np.int64)
    assert np.array_equal(fi, m["frame_index"][:m["frame_count"]])
    assert np.abs(fx["ref_normals"] - m["normals"])[kp].max() < 1e-12
    assert np.array_equal(fx["ref_flipped"][kf], m["flipped"][fi][kf])
    assert np.array_equal(fx["ref_frames"][kf], m["frames"][fi][kf].astype(np.float32))
    assert np.array_equal(fx["ref_mask"][kf], m["mask"][fi][kf])
    assert np.array_equal(fx["ref_pre_search"][kf], m["pre_search"][fi][kf])
    assert np.array_equal(fx["ref_pre_antipodal"][kf], m["pre_antipodal"][fi][kf])
    for k in ("search_score", "antipodal_score", "objects_label", "valid"):
        assert np.array_equal(fx["ref_" + k][kf], g[k][kf]), k
    from tests import local_search_ref as LR
    rows = fx["ref_valid_frame_rows"]
    want = LR.frames_of(fx["cloud"].T[fi[rows]], fx["ref_frames"][rows], PV.default_config().search)
    # the reference's fp32 torch.inverse and batched product against float64: coordinates below 2, a few 2^-23
    assert np.abs(fx["ref_valid_frame"] - want).max() < 1e-5


def test_fixture_holds_what_it_is_for(fx, base):
    m, g = base
    kp, kf = fx["keep_points"].astype(bool), fx["keep_frames"].astype(bool)
    assert (~kp).sum() <= 0.02 * len(kp) and (~kf).sum() <= 0.02 * len(kf)
    reason = g["reason"][kf]
    cand = m["candidate"] & kp
    have = {"valid": int((g["valid"] & kf).sum()), "flipped": int((m["flipped"] & cand).sum()),
            "unflipped": int((~m["flipped"] & cand).sum()), "unmatched": int(((m["nearest"] < 0) & kp).sum()),
            "region_only": int((m["region_only"] & kp).sum()), "reach": int((g["reach"] & kf).sum()),
            "reach_valid": int((g["reach"] & g["valid"] & kf).sum())}
    for i, name in enumerate(PV.REASONS):
        have[name] = int((reason == i).sum())
    for k, v in PV.REQUIRED.items():
        assert have[k] >= v, (k, have[k])
    # the pinned values: exactly 50, exactly float32(0.3) and the fp32 value below it, whole depths of zeros
    a03 = np.float32(0.3)
    assert (fx["rows_search"] == 50).sum() > 100 and (fx["rows_antipodal"] == a03).sum() > 100
    assert (fx["rows_antipodal"] == np.nextafter(a03, np.float32(0))).sum() > 100
    assert (fx["rows_search"] == 0).all(2).sum() > 100
    assert float(a03) > 0.3                      # what numpy's float64 comparison sees (:182)
    assert os.path.getsize(GOLDEN) <= (1 << 20)


@pytest.mark.parametrize("name", PV.SABOTAGES)
def test_fixture_sees_the_mistake(fx, base, name):
    assert PV.altered_rows(fx, name, base=base) >= 20


def test_frames_per_pass_is_the_kernels():
    assert PV.frames_per_pass_in_source() == PV.FRAMES_PER_PASS


def _cpu_scene(L, T, M=6):
    from s4g_release_amd.postprocess import DarbouxScene
    z = lambda *s: torch.zeros(*s)                                      # noqa: E731
    return DarbouxScene(z(3, M), z(3, M), z(M).int(), z(M, 3, 3), z(M, 3, 3), z(M, L, T).int(), z(M, L, T).int(),
                        z(M, L, T), z(M, L, T))


def test_no_cpu_fallback():
    from s4g_release_amd import postprocess as PP
    import s4g_release_amd as S
    cloud, cam = torch.zeros(3, 5), torch.zeros(3)
    for fn in (PP.label_precomputed_view, PP.match_scene_frames, S.label_precomputed_view, S.match_scene_frames):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            fn(cloud, cloud, _cpu_scene(4, 12), cam)
    for fn in (PP.grade_precomputed_frames, S.grade_precomputed_frames):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            fn(torch.zeros(2, 3), torch.zeros(2, 3, 3), torch.zeros(2, 4, 12, dtype=torch.bool),
               torch.zeros(2, 4, 12, dtype=torch.int32), torch.zeros(2, 4, 12), torch.zeros(3, 6),
               torch.zeros(6, dtype=torch.int32))


@pytest.mark.parametrize("L,T", [(9, 12), (4, 17)])
def test_compiled_maxima(L, T):
    """L <= 8 and T <= 16 are the compiled maxima: anything larger is a ValueError, before a tensor is looked at."""
    from s4g_release_amd import postprocess as PP
    search = PP.LocalSearchConfig(length_search=tuple(-0.01 * (i + 1) for i in range(L)),
                                  theta_search_deg=tuple(range(T)))
    cfg = PP.PrecomputedViewConfig(search=search)
    cloud, cam = torch.zeros(3, 5), torch.zeros(3)
    with pytest.raises(ValueError):
        PP.label_precomputed_view(cloud, cloud, _cpu_scene(L, T), cam, cfg)
    with pytest.raises(ValueError):
        PP.match_scene_frames(cloud, cloud, _cpu_scene(L, T), cam, cfg)
    with pytest.raises(ValueError):
        PP.grade_precomputed_frames(torch.zeros(2, 3), torch.zeros(2, 3, 3), torch.zeros(2, L, T, dtype=torch.bool),
                                    torch.zeros(2, L, T, dtype=torch.int32), torch.zeros(2, L, T), torch.zeros(3, 6),
                                    torch.zeros(6, dtype=torch.int32), cfg)


def test_config_defaults():
    cfg = PV.default_config()
    assert (cfg.search_threshold, cfg.antipodal_threshold, cfg.valid_search_min, cfg.valid_antipodal_min) == (50, 0.3, 1, 0.1)
    assert cfg.sample_region is None and cfg.region == cfg.search.table_height + 0.015
    assert PV.default_config(sample_region=0.9).region == 0.9
