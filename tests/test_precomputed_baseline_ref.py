"""CPU tests of the fast baseline labels: the fixture the reference's own `_find_match`, `finger_hand` and
`close_region_projection` produced (tests/golden/precomputed_baseline.npz, tools/gen_golden_precomputed_baseline.py)
against the float64 yardstick (tests/precomputed_baseline_ref.py), what the fixture must hold, the mistakes it must see,
the constants the GPU ladder follows, and the refusals of the public entry points, which need no GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import close_region_ref as CRR
from tests import precomputed_baseline_ref as PB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "precomputed_baseline.npz")


@pytest.fixture(scope="module")
def fx():
    return PB.load_fixture()


@pytest.fixture(scope="module")
def base(fx):
    return PB.label64(*PB.case_of(fx))


def test_fixture_equals_the_yardstick_on_kept_rows(fx, base):
    m, g = base
    cfg = PB.default_config()
    kp, kf = fx["keep_points"].astype(bool), fx["keep_frames"].astype(bool)
    ykp, ykf = PB.decided(m, g)
    assert np.array_equal(kp, ykp) and np.array_equal(kf, ykf)
    fi = fx["ref_frame_index"].astype(np.int64)
    assert np.array_equal(fi, m["frame_index"][:m["frame_count"]])
    assert np.abs(fx["ref_normals"] - m["normals"])[kp].max() < 1e-12
    assert np.array_equal(fx["ref_flipped"][kf], m["flipped"][fi][kf])
    assert np.array_equal(fx["ref_frames"][kf], m["frames"][fi][kf].astype(np.float32))
    assert np.array_equal(fx["ref_mask"][kf], m["mask"][fi][kf])
    assert np.array_equal(fx["ref_pre_antipodal"][kf], m["pre_antipodal"][fi][kf])
    assert np.array_equal(fx["ref_valid"][kf], g["valid"][kf])
    assert np.array_equal(fx["ref_score"][kf], g["score"][kf])
    assert np.array_equal(fx["ref_index"][kf], g["index"][kf].astype(np.int32))
    # the reference's fp32 product against float64: coordinates below 2, a few 2^-23
    assert np.abs(fx["ref_valid_frame"][kf] - g["g2l"][kf]).max() < 1e-5
    # crop sets: certain members in, ambiguous optional, nothing else; the stored sets and maps against float64
    vrows = np.nonzero(fx["ref_valid"])[0]
    off = fx["set_offset"]
    for k, f in enumerate(vrows):
        if not kf[f]:
            continue
        idx, r = fx["set_index"][off[k]:off[k + 1]], g["regions"][f]
        assert len(idx) == fx["ref_set_size"][f]
        assert set(r["certain"]) <= set(idx) <= set(r["certain"]) | set(r["ambiguous"]), f
    so = fx["stored_offset"]
    for k, f in enumerate(fx["stored_rows"]):
        p32, n32 = fx["stored_points"][:, so[k]:so[k + 1]], fx["stored_normals"][:, so[k]:so[k + 1]]
        idx = g["regions"][f]["certain"]
        assert not len(g["regions"][f]["ambiguous"]) and p32.shape[1] == len(idx)
        assert np.abs(p32 - g["regions"][f]["local"][:, idx]).max(initial=0.0) < CRR.TOL
        want_n = g["g2l"][f][:3, :3] @ g["normals32"][:, idx].astype(np.float64)
        assert np.abs(n32 - want_n).max(initial=0.0) < 1e-5
        m64, _ = CRR.projection64(p32, n32, cfg.projection, cfg.search)
        assert (np.abs(fx["maps"][k] - m64) <= CRR.map_bound(p32, n32, cfg.projection, cfg.search)).all(), f


def test_fixture_holds_what_it_is_for(fx, base):
    m, g = base
    kp, kf = fx["keep_points"].astype(bool), fx["keep_frames"].astype(bool)
    assert (~kp).sum() <= 0.02 * len(kp) and (~kf).sum() <= 0.02 * len(kf)
    vk = g["valid"] & kf
    assert (PB.ambiguous_crop(g) & vk).sum() <= 0.02 * vk.sum()
    assert np.array_equal(fx["ref_ambiguous_crop"], PB.ambiguous_crop(g))
    have = PB.counts(fx, m, g)
    for k, v in PB.REQUIRED.items():
        assert have[k] >= v, (k, have[k])
    assert len(fx["stored_rows"]) >= 20 and (fx["ref_set_size"][fx["stored_rows"]] > 0).sum() >= 10
    # the pinned values: exactly float32(0.3) and the fp32 value below it; the mask does not read the search scores
    a03 = np.float32(0.3)
    assert (fx["rows_antipodal"] == a03).sum() > 100 and (fx["rows_antipodal"] == np.nextafter(a03, np.float32(0))).sum() > 100
    assert float(a03) > 0.3                      # what numpy's float64 comparison sees (:178)
    assert (m["mask"] & (m["pre_search"] <= 50)).sum() > 100
    assert os.path.getsize(GOLDEN) < 1000000


@pytest.mark.parametrize("name", PB.SABOTAGES)
def test_fixture_sees_the_mistake(fx, base, name):
    assert len(PB.SABOTAGES) >= 12
    assert PB.altered_rows(PB.case_of(fx), name, base=base) >= 20


def test_frames_per_pass_is_the_kernels():
    gx, slots = PB.slots_in_source()
    assert (gx, slots) == (32, 20) and gx * slots == PB.FRAMES_PER_PASS


def _cpu_scene(L, T, M=6):
    from s4g_release_amd.postprocess import DarbouxScene
    z = lambda *s: torch.zeros(*s)                                      # noqa: E731
    return DarbouxScene(z(3, M), z(3, M), z(M).int(), z(M, 3, 3), z(M, 3, 3), z(M, L, T).int(), z(M, L, T).int(),
                        z(M, L, T), z(M, L, T))


def test_no_cpu_fallback():
    from s4g_release_amd import postprocess as PP
    import s4g_release_amd as S
    cloud, cam = torch.zeros(3, 5), torch.zeros(3)
    for fn in (PP.label_precomputed_baseline_view, S.label_precomputed_baseline_view):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            fn(cloud, cloud, _cpu_scene(4, 12), cam)
    for fn in (PP.grade_precomputed_baseline_frames, S.grade_precomputed_baseline_frames):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            fn(torch.zeros(2, 3), torch.zeros(2, 3, 3), torch.zeros(2, 4, 12, dtype=torch.bool), torch.zeros(2, 4, 12),
               torch.zeros(3, 6))
    for fn in (PP.score_projections, PP.score_close_regions):
        with pytest.raises(RuntimeError, match="PrecomputedBaselineLabels"):
            fn(object(), lambda *a, **k: None)


@pytest.mark.parametrize("L,T", [(9, 12), (4, 17)])
def test_compiled_maxima(L, T):
    """L <= 8 and T <= 16 are the compiled maxima: anything larger is a ValueError, before a tensor is looked at."""
    from s4g_release_amd import postprocess as PP
    search = PP.LocalSearchConfig(length_search=tuple(-0.01 * (i + 1) for i in range(L)),
                                  theta_search_deg=tuple(range(T)))
    cfg = PP.PrecomputedBaselineConfig(search=search)
    cloud, cam = torch.zeros(3, 5), torch.zeros(3)
    with pytest.raises(ValueError):
        PP.label_precomputed_baseline_view(cloud, cloud, _cpu_scene(L, T), cam, cfg)
    with pytest.raises(ValueError):
        PP.grade_precomputed_baseline_frames(torch.zeros(2, 3), torch.zeros(2, 3, 3),
                                             torch.zeros(2, L, T, dtype=torch.bool), torch.zeros(2, L, T),
                                             torch.zeros(3, 6), cfg)


def test_config_and_c_entries():
    from s4g_release_amd import _cabi
    from s4g_release_amd import postprocess as PP
    cfg = PB.default_config()
    assert cfg.antipodal_threshold == 0.3 and cfg.sample_region is None
    assert isinstance(cfg.search, PP.LocalSearchConfig) and isinstance(cfg.projection, PP.ProjectionConfig)
    v = cfg.view_config()
    assert v.search_threshold is None and v.antipodal_threshold == 0.3 and v.search is cfg.search
    assert v.region == cfg.search.table_height + 0.015 and PB.default_config(sample_region=0.9).view_config().region == 0.9
    assert PP.PrecomputedViewConfig().search_threshold == 50                 # the view stage's default is unchanged
    header = open(os.path.join(PB.ROOT, "include", "s4g_ops.h")).read()
    abi = header[header.index(" * 14:"):header.index("#define S4G_ABI_VERSION")]
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in (("s4g_precomputed_baseline_search_workspace_bytes", 5), ("s4g_precomputed_baseline_search_f32", 24)):
        assert name in abi and re.search(r"\b%s\s*\(" % name, code) and len(_cabi.SIGNATURES[name][1]) == nargs, name
    assert _cabi.S4G_ABI_VERSION == 14 and "#define S4G_ABI_VERSION 14" in header
