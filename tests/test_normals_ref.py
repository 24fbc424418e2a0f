"""The float64 yardstick of the normal estimation (tests/normals_ref.py) against closed forms and against the fixture
it produced (tests/golden/normals.npz: pinned by restatement only, open3d cannot run here), the C ABI's declarations,
and what the fixture can tell apart: each sabotage of the yardstick misses the bound the kernel is held to
(tests/test_normals_gpu.py) by at least 100 times on at least 20 rows of a fixture case.  No GPU."""
import os

import numpy as np
import pytest

from tests import golden_util as GU
from tests import match_normals_ref as MR
from tests import normals_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("r10", "r15", "lattice", "sphere")


@pytest.fixture(scope="module")
def fx():
    return GU.load("normals.npz")


def case_of(fx, name):
    """-> (cloud, camera, radius, max_nn, the stored yardstick result, margin) of a fixture case."""
    pre = name + "/" if name in ("lattice", "sphere") else ""
    y = {k: fx["%s/%s" % (name, k)] for k in ("normals", "count", "flags", "gap", "towards")}
    return (fx[pre + "cloud"], fx[pre + "camera"], float(fx[name + "/radius"][0]), int(fx[name + "/max_nn"][0]), y,
            float(fx[name + "/margin"][0]))


def test_the_cabi_declares_both_entries_and_the_header_names_them():
    from s4g_release_amd import _cabi
    header = open(os.path.join(ROOT, "include", "s4g_ops.h")).read()
    assert _cabi.S4G_ABI_VERSION == 14 and "#define S4G_ABI_VERSION 14" in header
    for name, nargs in (("s4g_estimate_normals_f32", 13), ("s4g_estimate_normals_workspace_bytes", 2)):
        assert name in _cabi.SIGNATURES and len(_cabi.SIGNATURES[name][1]) == nargs
        decl = header[header.rindex(name + "("):]                         # (the declaration follows its comment)
        assert decl[:decl.index(");")].count(",") == nargs - 1


@pytest.mark.parametrize("name", CASES)
def test_the_yardstick_reproduces_the_fixture(fx, name):
    cloud, camera, radius, max_nn, y, margin = case_of(fx, name)
    got = NR.normals_ref(cloud, camera, radius, max_nn)
    assert np.array_equal(got["count"], y["count"]) and np.array_equal(got["flags"], y["flags"])
    assert np.abs(got["normals"] - y["normals"]).max() <= 1e-12
    assert np.abs(got["gap"] - y["gap"]).max() <= 1e-9
    assert np.array_equal(MR.in_radius32(cloud, cloud, radius), got["inside"])       # the set is the pinned fp32 one
    n = cloud.shape[1]
    plane = y["count"] >= NR.FEW_BELOW
    # the cap the issue sets: at most 1 % of the rows left out for their gap, at most 2 % few
    assert (plane & (y["gap"] < 1e-3)).sum() <= 0.01 * n and ((y["flags"] & NR.FEW) != 0).sum() <= 0.02 * n
    assert 0 < margin < 1e-6
    # unit vectors that face the camera
    assert np.abs(np.linalg.norm(y["normals"], axis=1) - 1).max() < 1e-12
    assert ((y["normals"] * (camera.astype(np.float64) - cloud.astype(np.float64).T)).sum(1) >= 0).all()
    # the fp32 restatement is what the margin says it is
    y32 = NR.normals_ref(cloud, camera, radius, max_nn, dtype=np.float32)
    use = plane & (y["gap"] >= 1e-3)
    assert float((NR.row_error(y32["normals"], y) * y["gap"])[use].max()) == pytest.approx(margin, rel=1e-6)


def test_the_fixture_holds_what_it_is_for(fx):
    assert 2900 <= fx["cloud"].shape[1] <= 3100 and fx["lattice/cloud"].shape[1] == 400
    assert float(fx["r10/radius"][0]) == 0.01 and float(fx["r15/radius"][0]) == 0.015 and int(fx["r10/max_nn"][0]) == 30
    capped = {c: ((fx[c + "/flags"] & NR.CAPPED) != 0).mean() for c in CASES}
    assert capped["r10"] > 0.01 and capped["r15"] > 0.3 and capped["lattice"] > 0.5 and capped["sphere"] == 0
    assert os.path.getsize(os.path.join(GU.GOLDEN, "normals.npz")) <= 1 << 20


# ---- closed forms -------------------------------------------------------------------------------------------------

def plane_lattice(axis, side=9, step=1.0 / 64):
    a, b = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    pts = np.zeros((3, side * side))
    pts[(axis + 1) % 3], pts[(axis + 2) % 3] = a.ravel() * step, b.ravel() * step
    pts[axis] = 0.25
    return pts.astype(np.float32)


@pytest.mark.parametrize("axis", (0, 1, 2))
@pytest.mark.parametrize("side", (1.0, -1.0))
def test_an_axis_aligned_lattice_plane_gives_exactly_the_axis(axis, side):
    pts = plane_lattice(axis)
    cam = np.full(3, 0.05, np.float32)
    cam[axis] = 0.25 + side
    y = NR.normals_ref(pts, cam, 3.5 / 64, 30)
    e = np.zeros(3)
    e[axis] = side
    assert (y["normals"] == e).all() and (y["count"] >= 9).all() and (y["flags"] & ~NR.CAPPED == 0).all()
    # without a camera the leading component is positive
    assert (NR.normals_ref(pts, None, 3.5 / 64, 30)["normals"] == np.abs(e)).all()


def test_a_tilted_plane_is_within_the_rounding_of_its_points():
    rng = np.random.RandomState(3)
    n = np.array([0.3, -0.5, 0.81])
    n /= np.linalg.norm(n)
    u = np.cross(n, [1.0, 0, 0])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    ab = rng.uniform(-0.02, 0.02, (400, 2))
    pts = (np.array([0.1, 0.2, 0.7]) + ab[:, :1] * u + ab[:, 1:] * v).astype(np.float32).T
    y = NR.normals_ref(pts, np.array([0.1, 0.2, 0.7]) + n, 0.01, 30)
    plane = y["count"] >= 10
    assert plane.sum() > 300
    # fp32 rounding moves a point by at most 2^-24 * 0.75 off the plane; over a neighbourhood of spread >= 0.003 that
    # tilts the fit by at most a few 1e-5
    assert np.linalg.norm(y["normals"][plane] - n, axis=1).max() < 1e-4


def test_a_sphere_patch_points_along_the_radius():
    rng = np.random.RandomState(4)
    R, c = 0.5, np.array([0.0, 0.0, -1.0])
    d = rng.normal(size=(20000, 3)) * [0.05, 0.05, 0] + [0, 0, 1.0]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = (c + R * d).astype(np.float32).T
    y = NR.normals_ref(pts, c + [0, 0, 5.0], 0.01, 30, rows=range(0, 20000, 40))
    rows = np.arange(0, 20000, 40)
    rows = rows[y["count"][rows] == 30]
    assert len(rows) > 200
    # a neighbourhood of radius r on a sphere of radius R that is not centred on the query tilts the fitted plane by at
    # most about r / R
    assert np.linalg.norm(y["normals"][rows] - d[rows], axis=1).max() < 0.01 / R


def test_three_points_give_their_plane_and_a_line_gives_a_perpendicular():
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 2]], np.float64).T / 128
    y = NR.normals_ref(tri.astype(np.float32), None, 0.25, 30)
    want = np.array([0, 2, -1]) / np.sqrt(5.0)                  # no camera: the leading component, y, is positive
    assert (y["count"] == 3).all() and (y["flags"] == 0).all()
    assert np.abs(y["normals"] - want).max() < 1e-12
    line = (np.arange(5)[None, :] * np.array([[1.0], [2.0], [-1.0]]) / 128).astype(np.float32)
    y = NR.normals_ref(line, None, 0.25, 30)
    assert (y["count"] == 5).all() and (y["flags"] == 0).all()  # collinear is not degenerate
    assert np.abs(np.linalg.norm(y["normals"], axis=1) - 1).max() < 1e-12
    assert np.abs(y["normals"] @ np.array([1.0, 2.0, -1.0])).max() < 1e-12


def test_the_decisions():
    L = MR.lattice
    cam = np.array([0, 0, -4.0], np.float32)
    # two points: few, (0, 0, 1) turned towards the camera
    y = NR.normals_ref(L([[0, 0, 0], [1, 0, 0]]), cam, 0.25, 30)
    assert (y["flags"] == NR.FEW).all() and (y["normals"] == [0, 0, -1]).all() and (y["count"] == 2).all()
    # identical points: degenerate; copies at lower indices rank first, so max_nn = 3 keeps the first three everywhere
    y = NR.normals_ref(L([[1, 1, 1]] * 5), None, 0.25, 3)
    assert (y["flags"] == NR.DEGENERATE | NR.CAPPED).all() and (y["normals"] == [0, 0, 1]).all()
    assert (y["kept"] == [0, 1, 2]).all()
    # a point that is not finite is no neighbour and no query; padding is neither
    pts = L([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 2, 0]])
    pts[1, 3] = np.nan
    y = NR.normals_ref(pts, cam, 0.25, 30, live=4)
    assert list(y["flags"]) == [0, 0, 0, NR.NONFINITE, NR.PADDING] and list(y["count"]) == [3, 3, 3, 0, 0]
    assert (y["normals"][:3] == [0, 0, -1]).all() and (y["normals"][3] == [0, 0, 1]).all()
    assert (y["normals"][4] == 0).all()


# ---- sabotage -----------------------------------------------------------------------------------------------------

SABOTAGE = {"uncentred": "r10", "largest": "r10", "middle": "r10", "no cap": "r15", "cap by index": "r15",
            "non-strict": "sphere", "doubled radius": "r10", "no self": "r10", "threshold 5": "r10",
            "no orientation": "r10", "inverted orientation": "r10", "tie reversed": "lattice"}


def test_every_variant_has_a_case():
    assert sorted(SABOTAGE) == sorted(NR.VARIANTS)


@pytest.mark.parametrize("variant", NR.VARIANTS)
def test_the_fixture_catches(fx, variant):
    cloud, camera, radius, max_nn, y, margin = case_of(fx, SABOTAGE[variant])
    s = NR.normals_ref(cloud, camera, radius, max_nn, variant=variant)
    missed = NR.row_error(s["normals"], y) > 100.0 * NR.bound(y, margin)
    assert missed.sum() >= 20, (variant, int(missed.sum()))
