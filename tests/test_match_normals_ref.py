"""The float64 yardstick of the normal matching (tests/match_normals_ref.py) against the fixture the reference's own
`_find_normal` produced (tests/golden/match_normals.npz), the C ABI's declarations, and what the fixture can tell
apart: each sabotage of the yardstick moves a stated share of the fixture's queries by at least 100 times the bound
the kernel is held to (tests/test_match_normals_gpu.py).  No GPU."""
import inspect
import os

import numpy as np
import pytest

from tests import golden_util as GU
from tests import match_normals_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 4.0              # the GPU bound: |n - n64| * |m| <= FACTOR * margin


@pytest.fixture(scope="module")
def fx():
    return GU.load("match_normals.npz")


@pytest.fixture(scope="module")
def y(fx):
    return MR.normals64(fx["cloud"], fx["scene"], fx["scene_normals"], fx["camera"], float(fx["radius"][0]),
                        int(fx["max_nn"][0]))


def test_the_yardstick_reproduces_the_fixture(fx, y):
    keep, max_nn = fx["keep"], int(fx["max_nn"][0])
    assert np.array_equal(y["count"], fx["count"])
    assert np.array_equal(np.nonzero(MR.decided(y))[0], keep)             # the fixture keeps the decided queries
    assert np.abs(y["normals"][keep] - fx["normals"]).max() <= 1e-12
    n = len(fx["count"])
    capped, empty = (y["flags"] & MR.CAPPED) != 0, (y["flags"] & MR.EMPTY) != 0
    kept = np.zeros(n, bool)
    kept[keep] = True
    assert (kept & capped).sum() >= 300 and (kept & (y["in_radius"] >= 1) & (y["in_radius"] <= max_nn)).sum() >= 300
    assert empty.sum() >= 5 and n - len(keep) <= 0.02 * n
    live = kept & ~empty
    assert (live & y["flipped"]).any() and (live & ~y["flipped"]).any()
    assert np.array_equal(MR.in_radius32(fx["cloud"], fx["scene"], float(fx["radius"][0])), y["in_radius"])
    assert 0 < float(fx["margin"][0]) < 1e-6 and float(fx["radius"][0]) == 0.01 and max_nn == 30
    assert 14000 <= fx["scene"].shape[1] <= 16000 and 1400 <= n <= 1600
    # the reference's normals are unit vectors that face the camera; the empty queries got (0, 0, +-1)
    ref = fx["normals"]
    assert np.abs(np.linalg.norm(ref, axis=1) - 1).max() < 1e-12
    to_cam = fx["camera"].astype(np.float64) - fx["cloud"].astype(np.float64).T[keep]
    assert ((ref * to_cam).sum(1) >= 0).all()
    assert (np.abs(ref[empty[keep]]) == [0, 0, 1]).all()
    assert os.path.getsize(os.path.join(GU.GOLDEN, "match_normals.npz")) <= 1 << 20


def test_the_cabi_declares_both_entries_and_the_header_names_them():
    from s4g_release_amd import _cabi
    header = open(os.path.join(ROOT, "include", "s4g_ops.h")).read()
    for name, nargs in (("s4g_match_normals_f32", 15), ("s4g_match_normals_workspace_bytes", 3)):
        assert name in _cabi.SIGNATURES and len(_cabi.SIGNATURES[name][1]) == nargs
        decl = header[header.rindex(name + "("):]                         # (the declaration follows its comment)
        assert decl[:decl.index(");")].count(",") == nargs - 1
        assert name in header[:header.index("#define S4G_ABI_VERSION")]   # the ABI-14 list names it
    assert _cabi.S4G_ABI_VERSION == 14 and "#define S4G_ABI_VERSION 14" in header
    import s4g_release_amd
    from s4g_release_amd import postprocess as PP
    assert callable(s4g_release_amd.match_normals) and PP.NORMAL_MAX_NN == 30
    sig = inspect.signature(PP.label_view).parameters
    assert list(sig)[-3:] == ["match_normal", "camera", "max_nn"] and sig["match_normal"].default is False
    assert list(inspect.signature(PP.match_normals).parameters) == ["cloud", "scene_points", "scene_normals", "camera",
                                                                    "radius", "max_nn"]
    assert [f for f in PP.ViewLabels.__dataclass_fields__] == ["search", "darboux", "cloud_index", "matched"]
    assert PP.ViewLabels.__dataclass_fields__["matched"].default is None
    for prop in ("capped", "empty", "cancelled", "nonfinite"):
        assert isinstance(getattr(PP.MatchedNormals, prop), property)


def _moved(fx, y, other):
    """Share of the fixture's kept, non-empty queries on which `other` is at least 100 GPU bounds from the yardstick."""
    keep = fx["keep"][y["count"][fx["keep"]] > 0]
    bound = FACTOR * float(fx["margin"][0]) / y["mean_norm"][keep]
    return float((np.abs(other[keep] - y["normals"][keep]).max(1) >= 100 * bound).mean())


def _mean_of(fx, y, pick):
    """The yardstick's normalise-and-orient on the mean of the scene normals pick(i) -> indices chooses."""
    nrm = fx["scene_normals"].astype(np.float64).T
    q, cam = fx["cloud"].astype(np.float64).T, fx["camera"].astype(np.float64)
    out = y["normals"].copy()
    for i in np.nonzero(y["count"] > 0)[0]:
        m = nrm[pick(i)].mean(0)
        n = m / np.linalg.norm(m)
        out[i] = -n if n @ (cam - q[i]) < 0 else n
    return out


def _inside(fx, i, scale=1.0):
    q = fx["cloud"].astype(np.float64).T[i]
    d2 = ((fx["scene"].astype(np.float64).T - q) ** 2).sum(1)
    return np.nonzero(d2 < (scale * float(fx["radius"][0])) ** 2)[0]


def test_the_helper_restates_the_yardstick(fx, y):
    same = _mean_of(fx, y, lambda i: y["kept"][i][y["kept"][i] >= 0])
    assert np.abs(same - y["normals"]).max() <= 1e-12


def test_sabotage_no_cap(fx, y):
    """The mean over everything inside the radius: every capped query can move -- most do."""
    share = _moved(fx, y, _mean_of(fx, y, lambda i: _inside(fx, i)))
    print("no cap: %.1f %% of the kept queries moved" % (100 * share))
    assert share >= 0.5


def test_sabotage_first_by_index(fx, y):
    """The first 30 by index instead of the 30 nearest."""
    share = _moved(fx, y, _mean_of(fx, y, lambda i: _inside(fx, i)[:int(fx["max_nn"][0])]))
    print("first by index: %.1f %% of the kept queries moved" % (100 * share))
    assert share >= 0.5


def test_sabotage_no_orientation(fx, y):
    """Without the orientation every flipped query is off by 2."""
    other = MR.normals64(fx["cloud"], fx["scene"], fx["scene_normals"], None, float(fx["radius"][0]),
                         int(fx["max_nn"][0]))["normals"]
    share = _moved(fx, y, other)
    keep = fx["keep"][y["count"][fx["keep"]] > 0]
    print("no orientation: %.1f %% of the kept queries moved" % (100 * share))
    assert share == y["flipped"][keep].mean() and share >= 0.2


def test_sabotage_radius_half_as_large_again(fx, y):
    """Radius 1.5 r: the queries with fewer than 30 neighbours gain some."""
    other = MR.normals64(fx["cloud"], fx["scene"], fx["scene_normals"], fx["camera"], 1.5 * float(fx["radius"][0]),
                         int(fx["max_nn"][0]))["normals"]
    share = _moved(fx, y, other)
    print("radius x 1.5: %.1f %% of the kept queries moved" % (100 * share))
    assert share >= 0.2


@pytest.mark.parametrize("name", sorted(MR.edge_cases()))
def test_the_yardsticks_own_edge_cases(name):
    """A self-test of the yardstick alone on constructions whose answer is known by hand."""
    cloud, scene, nrm, cam, max_nn, expect = MR.edge_cases()[name]
    y = MR.normals64(cloud, scene, nrm, cam, 0.25, max_nn)
    assert list(y["count"]) == expect["count"] and list(y["flags"]) == expect["flags"], name
    assert np.abs(y["normals"] - np.asarray(expect["normals"], np.float64)).max() <= 1e-15, name
    assert MR.decided(y).all() or name.startswith("tie") or name == "at r"


def test_the_yardstick_on_values_that_are_not_finite():
    L = MR.lattice
    cloud = L([[0, 0, 0], [0, 0, 0], [64, 0, 0]])
    cloud[0, 1] = np.nan
    scene = L([[1, 0, 0], [2, 0, 0], [65, 0, 0], [66, 0, 0]])
    scene[1, 1] = np.inf                                                   # never a neighbour
    nrm = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0], [0, np.nan, 0]], np.float32).T.copy()
    y = MR.normals64(cloud, scene, nrm, np.array([0, 0, 4], np.float32), 0.25, 30)
    assert list(y["count"]) == [1, 0, 2]
    assert list(y["flags"]) == [0, MR.EMPTY | MR.NONFINITE, MR.NONFINITE]
    assert (y["normals"][:2] == [0, 0, 1]).all() and np.isnan(y["normals"][2]).all()
