"""The float64 yardstick of the PointNetGPD classifier (tests/pointnet_gpd_ref.py) and the reference-shaped
`baselines.PointNetGPDClassifier` against the fixture the reference's own network produced
(tests/golden/pointnet_gpd.npz, tools/gen_golden_pointnet_gpd.py).

Bound: max(10 * margin, 1e-5) of each tensor's scale, margin being the reference's own fp32 distance from float64 that
the generator measured (4e-7 .. 2.7e-6).  A sabotaged network must miss the logits by at least 100 times that."""
import os
import re

import numpy as np
import pytest
import torch

from tests import pointnet_gpd_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("s4g_pngpd_pack_bytes", "s4g_pngpd_pack_f32", "s4g_pngpd_workspace_bytes", "s4g_pngpd_forward_f32")


@pytest.fixture(scope="module")
def fx():
    return PR.load_fixture()


@pytest.fixture(scope="module")
def want(fx):
    """(state, sets, float64 levels), computed once."""
    state, sets = PR.fixture_state(fx), PR.fixture_sets()
    return state, sets, PR.forward64(state, sets)


def _bound(fx, level):
    return max(10.0 * float(fx["margin/" + level][0]), 1e-5)


def test_fixture_is_small_and_complete(fx):
    assert os.path.getsize(PR.GOLDEN) < 1 << 20
    sizes = [int(n) for n in fx["set_sizes"]]
    assert len(sizes) == 29 and sizes[26:] == [1, 2, 1024]
    assert min(sizes[:26]) == 159 and max(sizes[:26]) == 1300 and sum(n > 900 for n in sizes[:26]) == 2
    assert [s.shape[1] for s in PR.fixture_sets()] == sizes
    for k, shape in (("logits", (29, 3)), ("hidden", (29, 256)), ("trans", (29, 3, 3)), ("global", (29, 1024)),
                     ("stn_global", (29, 1024))):
        assert fx[k].shape == shape and fx[k].dtype == np.float32 and "margin/" + k in fx
    stats = [k for k in fx if k.startswith("stat/")]
    assert len(stats) == 30 and sum(fx[k].size for k in stats if k.endswith("running_var")) == 3968


def test_hashes_are_closed_form():
    st = PR.hashed_state(3)
    assert st["feat.stn.conv3.weight"].shape == (1024, 128, 1) and st["fc3.weight"].shape == (3, 256)
    assert abs(float(np.abs(st["fc1.weight"]).max()) - np.sqrt(3 / 1024)) < 1e-4
    assert PR.hashed_state(5)["fc3.weight"].shape == (5, 256)
    assert np.array_equal(PR.hashed_state(5)["fc3.weight"][:3], st["fc3.weight"])      # element i depends on i alone
    assert not np.array_equal(PR.hashed_state(3, salt=1)["fc1.weight"], st["fc1.weight"])
    assert np.array_equal(PR.hashed_set(10, 4)[0], PR.hashed_set(5, 4).reshape(-1)[:10])


def test_yardstick_matches_the_reference(fx, want):
    for level in PR.LEVELS:
        d = PR.distance(fx[level], want[2][level])
        assert d <= _bound(fx, level), (level, d)


@pytest.mark.parametrize("sabotage", PR.SABOTAGES)
def test_sabotaged_yardsticks_miss(fx, want, sabotage):
    assert len(PR.SABOTAGES) >= 9
    state, sets, _ = want
    miss = PR.distance(fx["logits"], PR.forward64(state, sets, sabotage)["logits"])
    assert miss >= 100.0 * _bound(fx, "logits"), (sabotage, miss)


def test_module_matches_the_reference(fx, want):
    from s4g_release_amd.baselines import PointNetGPDClassifier, build_pointnetgpd
    state, sets, w = want
    net = build_pointnetgpd(3)
    assert isinstance(net, PointNetGPDClassifier)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(n) for n in fx["state_names"]]
    for v, shp in zip(sd.values(), fx["state_shapes"]):
        assert list(v.shape) == [int(s) for s in shp[:v.dim()]] and not shp[v.dim():].any()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    net.eval()
    with torch.no_grad():
        for i in range(len(sets)):
            got = net.features(torch.from_numpy(sets[i][None]))
            for level in PR.LEVELS:
                d = PR.distance(got[level][0].numpy(), w[level][i]) * float(np.abs(w[level][i]).max()) / float(
                    np.abs(w[level]).max())
                assert d <= _bound(fx, level), (i, level, d)
        same = np.stack([sets[27], sets[27][:, ::-1]])                      # (2, 3, 2): a set and its permutation
        got3 = net({"close_region_points": torch.from_numpy(same)})["grasp_logits"].numpy()
        got4 = net({"close_region_points": torch.from_numpy(same[None])})["grasp_logits"].numpy()
    assert got3.shape == (2, 3) and np.array_equal(got3, got4)
    assert PR.distance(got3[0], w["logits"][27]) <= _bound(fx, "logits") * float(np.abs(w["logits"]).max()) / float(
        np.abs(w["logits"][27]).max())
    assert np.allclose(got3[0], got3[1], atol=1e-5)
    with pytest.raises(RuntimeError):
        net({"close_region_points": torch.zeros(3, 5)})


def test_build_model_keeps_refusing_pointnetgpd():
    from s4g_release_amd import model
    with pytest.raises(ValueError):
        model.build_model("PointNetGPD")


def test_header_names_the_entry_points_under_abi_14():
    from s4g_release_amd import _cabi
    text = open(os.path.join(ROOT, "include", "s4g_ops.h")).read()
    assert re.search(r"#define S4G_ABI_VERSION 14\b", text) and _cabi.S4G_ABI_VERSION == 14
    start = text.index("\n * 14:")
    listed = text[start:text.index("*/", start)]
    for name in ENTRY_POINTS:
        assert name in listed, name
        assert re.search(r"\b(size_t|int) %s\(" % name, text), name
        assert name in _cabi.SIGNATURES
    assert os.path.exists(os.path.join(ROOT, "s4g_release_amd", "csrc", "pointnet_gpd.hip"))


def test_host_checks():
    """Everything FusedPointNetGPD and score_close_regions refuse before they touch a device."""
    import s4g_release_amd as pkg
    from s4g_release_amd import postprocess as PP
    from s4g_release_amd.baselines import FusedPointNetGPD, PointNetGPDClassifier
    assert pkg.build_pointnetgpd(4).out_channels == 4
    with pytest.raises(ValueError):
        FusedPointNetGPD(PointNetGPDClassifier(3, 17))
    with pytest.raises(ValueError):
        FusedPointNetGPD(PointNetGPDClassifier(4, 3))
    with pytest.raises(RuntimeError):
        FusedPointNetGPD(torch.nn.Linear(2, 2))
    run = FusedPointNetGPD(PointNetGPDClassifier(3, 3).eval())
    with pytest.raises(RuntimeError, match="CUDA"):
        run(torch.zeros(2, 3, 60))
    with pytest.raises(RuntimeError, match="CUDA"):
        run(np.zeros((2, 3, 60), np.float32))
    with pytest.raises(RuntimeError):
        PP.score_close_regions(object(), run)
    with pytest.raises(RuntimeError):
        pkg.score_close_regions(None, run)
    assert "score_close_regions" in pkg.__doc__
